"""CPU checks of the detector's object columns and segmentation map: the numpy restatement
(tests/detect_objects_oracle.py) on painted shapes with closed-form moments, the singular rule, the four flag bits each with a
control, the segmap against scipy.ndimage.label, the host derivation of the ellipse, extract_objects and
iterative_catalogue(detect_shapes=True) on stand-ins, the Python refusals and the C ABI.  No GPU is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import scipy.ndimage

from tests import detect_objects_oracle as oo
from tests import detect_shapes as ds
from tests import stub_detect_objects_engine as stub
from tests import test_iterative_batch_host as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 60
KW = ds.weighted_kwargs(dict(minarea=1))                 # the painted regime: back == 0, D == v == the painted integers


def _painted(data, weights=None, **kw):
    w = np.ones_like(data) if weights is None else weights
    exp, obj, details = oo.detect_weighted(data, w, **{**KW, **kw})
    assert (exp["back"] == 0.0).all() and np.array_equal(exp["D"][oo.counting(w)], data[oo.counting(w)])
    return exp, obj, details


def _counts_match(exp, obj):
    """for every object the pixels numbered k + 1 are its npix; nothing else is numbered"""
    n = len(exp["npix"])
    assert np.array_equal(np.bincount(obj["segmap"].ravel(), minlength=n + 1)[1:], exp["npix"])
    assert np.array_equal(obj["npix"], exp["npix"]) and obj["segmap"].max(initial=0) == n
    assert ((obj["segmap"] > 0) == (exp["labels"] >= 0)).all()


def test_rectangle_and_diagonal_bar_have_their_closed_form_moments():
    from debvader_amd import engine as E

    d = np.zeros((H, W))
    d[10:15, 20:29] = 3.0                                    # 9 wide, 5 high: x2 = (81 - 1) / 12, y2 = (25 - 1) / 12
    n, m = 12, 3                                             # the pixels (r, c) = (30 + i - j, 10 + i + j): a 45 degree bar
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    d[30 + i - j, 10 + i + j] = 2.0
    exp, obj, _ = _painted(d)
    assert len(exp["x"]) == 2 and obj["flag"].tolist() == [0, 0]
    _counts_match(exp, obj)
    A, B = (n * n - 1) / 12.0, (m * m - 1) / 12.0            # the variances along i and along j
    want = dict(x_iso=[24.0, 10 + (n - 1) / 2 + (m - 1) / 2], y_iso=[12.0, 30 + (n - 1) / 2 - (m - 1) / 2],
                x2=[80 / 12.0, A + B], y2=[24 / 12.0, A + B], xy=[0.0, A - B], dflux=[135.0, 72.0])
    for k, v in want.items():
        np.testing.assert_allclose(obj[k], v, rtol=0, atol=1e-12, err_msg=k)
    shape = dict(a=[np.sqrt(80 / 12.0), np.sqrt(2 * A)], b=[np.sqrt(2.0), np.sqrt(2 * B)], theta=[0.0, np.pi / 4])
    for derive in (oo.derived, E.detect_object_shapes):
        got = derive(obj["x2"], obj["y2"], obj["xy"])
        for k, v in shape.items():
            np.testing.assert_allclose(got[k], v, rtol=0, atol=1e-12, err_msg=k)
        det = obj["x2"] * obj["y2"] - obj["xy"] ** 2
        np.testing.assert_allclose(got["cxx"], obj["y2"] / det, rtol=1e-15)
        np.testing.assert_allclose(got["cyy"], obj["x2"] / det, rtol=1e-15)
        np.testing.assert_allclose(got["cxy"], -2 * obj["xy"] / det, rtol=1e-15)
        # SExtractor's ellipse: cxx dx^2 + cyy dy^2 + cxy dx dy = 1 at the end of the major axis
        ex, ey = got["a"] * np.cos(got["theta"]), got["a"] * np.sin(got["theta"])
        np.testing.assert_allclose(got["cxx"] * ex * ex + got["cyy"] * ey * ey + got["cxy"] * ex * ey, 1.0, rtol=1e-12)
    assert obj["xmin"].tolist() == [20, 10] and obj["xmax"].tolist() == [28, 10 + n - 1 + m - 1]
    assert obj["ymin"].tolist() == [10, 30 - (m - 1)] and obj["ymax"].tolist() == [14, 30 + n - 1]
    # flat tops: both peaks lie at the first pixel in raster order
    assert (obj["xpeak"].tolist(), obj["ypeak"].tolist()) == ([20, 12], [10, 28])
    assert (obj["xvpeak"].tolist(), obj["yvpeak"].tolist()) == ([20, 12], [10, 28]) and obj["vpeak"].tolist() == [3.0, 2.0]
    z = E.detect_object_shapes([1.0], [1.0], [0.0])
    assert z["theta"][0] == 0.0 and z["a"][0] == 1.0 and z["b"][0] == 1.0


def test_single_row_object_takes_the_singular_rule():
    d = np.zeros((H, W))
    d[20, 10:21] = 2.0                                       # 11 x 1: y2 = 0, x2 = 120 / 12
    d[30:34, 30:34] = 2.0                                    # the control
    d[40, 40] = 5.0                                          # one pixel: x2 = y2 = 0
    exp, obj, _ = _painted(d)
    assert obj["flag"].tolist() == [oo.SINGULAR, 0, oo.SINGULAR]
    assert obj["x2"][0] == 10.0 + 1.0 / 12.0 and obj["y2"][0] == 1.0 / 12.0 and obj["xy"][0] == 0.0
    assert obj["x2"][1] == 15 / 12.0 and obj["y2"][1] == 15 / 12.0
    assert obj["x2"][2] == 1.0 / 12.0 and obj["y2"][2] == 1.0 / 12.0
    _counts_match(exp, obj)


def test_bit_1_marks_the_objects_of_a_split_component():
    d = np.zeros((H, W))
    d[8:20, 6:40] = 1.0
    d[10:18, 8:18] = 5.0
    d[10:18, 26:38] = 6.0
    d[30:36, 10:20] = 4.0                                    # the control: one object
    exp, obj, details = _painted(d, minarea=4)
    assert [len(c["peak_pixels"]) for c in details] == [2, 1]
    assert (obj["flag"] & oo.BLENDED).tolist() == [1, 1, 0]
    _counts_match(exp, obj)
    # the two halves of the base are told apart by the segmap, which the labels cannot do
    assert set(np.unique(obj["segmap"][8:20, 6:40])) == {1, 2} and len(np.unique(exp["labels"][8:20, 6:40])) == 1
    assert obj["segmap"][12, 10] == 1 and obj["segmap"][12, 30] == 2 and (obj["segmap"][30:36, 10:20] == 3).all()


def test_bit_2_marks_the_objects_at_the_border():
    d = np.zeros((H, W))
    d[5:9, 0:4] = 2.0                                        # column 0
    d[20:24, 20:24] = 2.0                                    # the control
    d[H - 3:H, 30:34] = 2.0                                  # the last row
    d[30:34, W - 2:W] = 2.0                                  # the last column
    d[0:2, 40:44] = 2.0                                      # row 0
    d[12:16, 1:5] = 2.0                                      # one pixel off the border: not set
    exp, obj, _ = _painted(d)
    order = np.argsort(exp["parent"])
    assert np.array_equal(order, np.arange(6))
    assert (obj["flag"] & oo.BORDER).tolist() == [2, 2, 0, 0, 2, 2]
    _counts_match(exp, obj)


def test_bit_8_marks_the_objects_next_to_a_pixel_that_does_not_count():
    d = np.zeros((H, W))
    d[10:14, 10:14] = 2.0
    d[10:14, 30:34] = 2.0                                    # the control
    d[30:34, 10:14] = 2.0
    d[30:34, 30:34] = 2.0
    w = np.ones((H, W))
    w[14, 14] = 0.0                                          # the corner neighbour of (13, 13)
    w[29, 12] = np.inf                                       # above (30, 12)
    w[32, 36] = np.nan                                       # two columns off the last object: not a neighbour
    exp, obj, details = _painted(d, weights=w)
    assert (obj["flag"] & oo.MASKED).tolist() == [8, 0, 8, 0]
    # the same objects without a weight plane, as the unweighted call has them: the bit belongs to the weighted calls
    o2 = oo.objects(details, exp["D"], exp["v"])
    assert len(o2["flag"]) == 4 and (o2["flag"] & oo.MASKED).tolist() == [0, 0, 0, 0]
    _counts_match(exp, obj)
    # an object at the corner of the field asks only about the neighbours inside it
    d3 = np.zeros((H, W))
    d3[0:3, 0:3] = 2.0
    assert _painted(d3)[1]["flag"].tolist() == [oo.BORDER]


def test_segmap_of_unsplit_components_is_scipys_label_map():
    rng = np.random.default_rng(5)
    d = np.zeros((H, W))
    for _ in range(14):
        r, c = rng.integers(0, H - 6), rng.integers(0, W - 8)
        d[r:r + rng.integers(2, 6), c:c + rng.integers(2, 8)] = 3.0          # flat: nothing splits
    exp, obj, details = _painted(d, minarea=1)
    assert all(len(c["peak_pixels"]) == 1 for c in details) and len(details) >= 6
    lab, n = scipy.ndimage.label(d > 0.5, structure=np.ones((3, 3), bool))
    assert n == len(details) and np.array_equal(obj["segmap"], lab)
    _counts_match(exp, obj)


@pytest.mark.parametrize("name", ["comb", "nested_mesas", "plateaus", "row_wrap", "insignificant"])
def test_painted_cases_number_every_pixel_of_every_object(name):
    data, exp, details, _ = ds.oracle(name)
    obj = oo.objects(details, exp["D"], exp["v"], wt=np.ones_like(data))
    _counts_match(exp, obj)
    assert not (obj["flag"] & oo.MASKED).any()
    split = np.concatenate([[len(c["peak_pixels"]) > 1] * len(c["peak_pixels"]) for c in details])
    assert np.array_equal((obj["flag"] & oo.BLENDED) > 0, split)
    # peak of the catalogue at (xpeak, ypeak); the box holds exactly the numbered pixels
    assert np.array_equal(exp["D"][obj["ypeak"], obj["xpeak"]], exp["peak"])
    for k in range(len(exp["x"])):
        r, c = np.nonzero(obj["segmap"] == k + 1)
        assert (c.min(), c.max(), r.min(), r.max()) == (obj["xmin"][k], obj["xmax"][k], obj["ymin"][k], obj["ymax"][k])


def test_noisy_scenes_have_both_values_of_bit_8_and_hold_the_premises():
    """what tests/test_gpu_detect_objects.py asserts first, on the restatement alone"""
    from tests import detect_multiband_oracle as mo
    from tests import detect_weighted_oracle as wo

    data, weights, _, _ = wo.scene()
    exp, obj, details = oo.detect_weighted(data, weights, back_size=32)
    oo.check_p3_p4(details)
    assert (obj["flag"] & oo.MASKED).any() and not (obj["flag"] & oo.MASKED).all()
    _counts_match(exp, obj)
    fields, _ = mo.scene()
    planes = mo.variance_planes()
    planes[40:42, 32:34, :] = 0.0                            # a defect beside the r_only source
    exp, obj, details = oo.detect_multiband(fields, planes=planes, noise="absolute", thresh=mo.THRESH, back_size=mo.BACK_SIZE)
    oo.check_p3_p4(details)
    assert (obj["flag"] & oo.MASKED).any() and not (obj["flag"] & oo.MASKED).all()
    _counts_match(exp, obj)


def test_extract_objects_returns_seps_columns_and_the_pair():
    from debvader_amd.detect import detection

    names = ["npix", "xmin", "xmax", "ymin", "ymax", "x", "y", "x2", "y2", "xy", "a", "b", "theta", "cxx", "cyy", "cxy", "flux",
             "peak", "xpeak", "ypeak", "flag", "parent", "dflux", "vpeak", "xvpeak", "yvpeak", "x_iso", "y_iso"]
    dt = detection.object_dtype()
    assert list(dt.names) == names
    ints = {"npix", "xmin", "xmax", "ymin", "ymax", "xpeak", "ypeak", "flag", "parent", "xvpeak", "yvpeak"}
    assert all(dt[k] == (np.int32 if k in ints else np.float64) for k in names)
    img = np.zeros((2, 8, 9, 3))
    ctx = stub.RecordingContext()
    recs = detection.extract_objects_batch(img, ctx=ctx, thresh=2.0)
    assert ctx.shape == (2, 8, 9) and ctx.kw == dict(segmentation_map=False, thresh=2.0)
    assert [len(r) for r in recs] == [2, 1] and all(isinstance(r, np.recarray) and r.dtype == dt for r in recs)
    full = ctx.scene_detect_objects(img[:, :, :, 2])
    for k in names:
        np.testing.assert_array_equal(np.concatenate([r[k] for r in recs]), full[k], err_msg=k)
    rec, seg = detection.extract_objects(img, ctx=ctx, segmentation_map=True)
    assert ctx.shape == (1, 8, 9) and seg.shape == (8, 9) and seg.dtype == np.int32 and len(rec) == 2
    recs, segs = detection.extract_objects_batch(img, ctx=ctx, segmentation_map=True, weights=np.ones((2, 8, 9, 3)))
    assert segs.shape == (2, 8, 9) and ctx.kw["weights"].shape == (2, 8, 9)
    # several bands: the whole fields go down, planes indexed by the selection
    detection.extract_objects(img, ctx=ctx, bands=[0, 2], band_weights=[1.0, 2.0], weights=np.ones((2, 8, 9, 3)))
    assert ctx.shape == (1, 8, 9, 3) and ctx.kw["bands"] == [0, 2] and ctx.kw["weights"].shape == (1, 8, 9, 2)
    with pytest.raises(ValueError):
        detection.extract_objects(img, ctx=ctx, band_weights=[1.0])
    with pytest.raises(ValueError):
        detection.extract_objects(img[0], ctx=ctx)
    # object_records derives the ellipse where the result has none
    bare = {k: v for k, v in full.items() if k not in ("a", "b", "theta", "cxx", "cyy", "cxy")}
    np.testing.assert_array_equal(detection.object_records(bare)["a"], full["a"])


def test_python_refusals_come_before_the_library():
    from debvader_amd import engine as E

    f = np.zeros((1, 8, 9))
    call = E.Context.scene_detect_objects
    for bad in (dict(thresh=-0.5), dict(thresh=np.nan), dict(columns=False), dict(bands=[0]), dict(band_weights=[1.0]),
                dict(noise="absolute"), dict(filter_type="matched"), dict(weights=np.ones((1, 8, 8))),
                dict(weights=np.ones((1, 8, 9)), thresh=0.0), dict(minarea=0), dict(back_size=65)):
        with pytest.raises(ValueError):
            call(None, f, **bad)                              # (self is not reached)
    f4 = np.zeros((1, 8, 9, 3))
    for bad in (dict(thresh=0.0), dict(thresh=-1.0), dict(bands=[3]), dict(bands=[1, 1]), dict(band_weights=[1.0]),
                dict(noise="relative"), dict(weights=np.ones((1, 8, 9)))):
        with pytest.raises(ValueError):
            call(None, f4, **bad)
    with pytest.raises(ValueError):
        call(None, np.zeros((8, 9)))
    f[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        call(None, f)

    class Handle:                                             # a FieldSet whose handle must not be used
        shape = (1, 8, 8, 3)
        _detect_objects = (True, False)

        def _handle(self):
            return None

    with pytest.raises(ValueError, match=">= 0"):
        E.FieldSet.detect(Handle(), thresh=-1.0)


def test_parameter_lists_of_the_existing_calls_are_unchanged():
    from debvader_amd import engine as E
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch
    from debvader_amd.detect import detection

    par = lambda f: list(inspect.signature(f).parameters)        # noqa: E731
    tail = ["thresh", "minarea", "nthresh", "cont", "filter_kernel", "back_size", "back_filter"]
    assert par(E.Context.scene_detect) == ["self", "fields_r"] + tail + ["return_maps", "workspace_bytes", "weights", "mask",
                                                                        "noise", "filter_type"]
    assert par(E.Context.scene_detect_multiband) == ["self", "fields", "bands", "band_weights"] + tail + [
        "return_maps", "workspace_bytes", "weights", "mask", "noise", "filter_type"]
    assert par(E.FieldSet.detect) == ["self", "active"] + tail + ["workspace_bytes"]
    assert par(E.Context.scene_detect_objects)[:-1] == ["self", "fields", "bands", "band_weights"] + tail + [
        "workspace_bytes", "weights", "mask", "noise", "filter_type", "segmentation_map"]
    assert par(E.FieldSet.set_detect_objects) == ["self", "on", "segmentation_map"]
    assert par(detection.detect_objects) == ["field_image", "ctx", "bands", "band_weights", "kw"]
    assert par(detection.extract_objects) == ["field_image", "ctx", "bands", "band_weights", "segmentation_map", "kw"]
    assert par(detection.extract_objects_batch) == ["field_images", "ctx", "bands", "band_weights", "segmentation_map", "kw"]
    names = par(IterativeDeblendFieldBatch.iterative_catalogue)
    at = names.index("detect_shapes")
    assert names[at - 1] == "min_pivot" and names[at + 1] == "detect_bands" and names[-1] == "fit_groups"
    assert inspect.signature(IterativeDeblendFieldBatch.iterative_catalogue).parameters["detect_shapes"].default is False
    assert par(IterativeDeblendFieldBatch.iterative_deblending) == ["self", "mse_criterion", "mode", "max_iterations"]


def test_iterative_catalogue_carries_the_detection_of_every_row():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    script = [[(3, 1), (4, 0), (2, 0)], [(2, 2), (1, 0)]]
    obj, eng = stub.batch(script)
    res = obj.iterative_catalogue(detect_shapes=True, detect_thresh=2.0)
    names = [c[0] for c in eng.calls]
    assert names.count("set_detect_objects") == 1 and eng.calls[names.index("set_detect_objects")][1:] == (True, False)
    assert names.index("open") < names.index("set_detect_objects") < names.index("detect")
    det_names = [n for n, _ in IterativeDeblendFieldBatch.DETECT_COLUMNS]
    assert det_names == ["det_npix", "det_peak", "det_flux", "det_x", "det_y", "det_xmin", "det_xmax", "det_ymin", "det_ymax",
                         "det_x2", "det_y2", "det_xy", "det_a", "det_b", "det_theta", "det_flag"]
    plain, ref, core = bh._run(script)
    for m, (a, b) in enumerate(zip(res, ref)):
        assert list(a.dtype.names) == list(b.dtype.names) + det_names             # behind all other columns
        assert [len(r) for r in res] == [9, 3]
        for name in b.dtype.names:                                                # the shared columns: the run without
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[name], b[name])), name
        # the rows of pass k are the detections `kept` names: the valid ones stand first in the scripted catalogue, the
        # field's rows start behind those of the fields before it
        at = 0
        for k, (valid, invalid) in enumerate(script[m]):
            before = sum(sum(script[f][k]) for f in range(m) if k < len(script[f]))
            rows = before + np.arange(valid)
            total = sum(sum(script[f][k]) for f in range(len(script)) if k < len(script[f]))
            for name in stub.DET:
                np.testing.assert_array_equal(a["det_" + name][at:at + valid], stub.scripted_column(name, k, total)[rows],
                                              err_msg=name)
            np.testing.assert_array_equal(a["det_x"][at:at + valid], 40.0 + (np.arange(valid) - 3) + 0.2)
            at += valid
        assert a["det_npix"].dtype == np.int32 and a["det_flag"].dtype == np.int32 and a["det_x2"].dtype == np.float64
    assert obj.mse == plain.mse
    # without the keyword: the calls of the loop as it was
    obj2, eng2 = stub.batch(script)
    same = obj2.iterative_catalogue()
    assert "set_detect_objects" not in [c[0] for c in eng2.calls]
    assert [c[0] for c in eng2.calls] == [c[0] for c in core.engine.calls]
    assert [c[0] for c in eng.calls if c[0] != "set_detect_objects"] == [c[0] for c in core.engine.calls]
    assert all(list(a.dtype.names) == list(b.dtype.names) for a, b in zip(same, ref))
    # refused before the set is opened
    obj3, eng3 = stub.batch(script)
    with pytest.raises(ValueError, match=">= 0"):
        obj3.iterative_catalogue(detect_shapes=True, detect_thresh=-1.0)
    assert eng3.calls == []
    # a run that deblends nothing still has the columns
    obj4, _ = stub.batch([[(0, 0)]])
    assert list(obj4.iterative_catalogue(detect_shapes=True)[0].dtype.names)[-16:] == det_names


def test_header_export_map_and_ctypes_signatures():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    m = re.search(r"typedef struct dv_detect_objects \{([^}]*)\} dv_detect_objects;", header)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1))
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            t = "int32_t" if decl.startswith("int32_t") else "double"
            assert decl.startswith(t)
            fields += [(n.replace("*", "").strip(), t) for n in decl[len(t):].split(",")]
    want = [(k, "int32_t") for k in _lib.DETECT_OBJECT_INT] + [(k, "double") for k in _lib.DETECT_OBJECT_DOUBLE] + [
        ("segmap", "int32_t")]
    assert fields == want
    assert [(n, "int32_t" if t is C.POINTER(C.c_int32) else "double") for n, t in _lib.DvDetectObjects._fields_] == want
    assert C.sizeof(_lib.DvDetectObjects) == 17 * 8
    assert _lib.DETECT_OBJECT_INT == oo.INT_KEYS and _lib.DETECT_OBJECT_DOUBLE == oo.DOUBLE_KEYS
    for name, val in (("BLENDED", 1), ("BORDER", 2), ("SINGULAR", 4), ("MASKED", 8)):
        assert re.search(r"#define DV_DETECT_FLAG_%s %d\b" % (name, val), header), name
        assert getattr(_lib, "DETECT_FLAG_" + name) == val == getattr(oo, name)
    m = re.search(r"\bint dv_scene_detect_objects\(dv_ctx\* ctx,([^;]*)\);", header)
    assert m and re.search(r"const dv_detect_weights\* weights,\s*const dv_detect_bands\* bands,\s*"
                           r"const dv_detect_objects\* objects$", m.group(1).strip())
    assert re.search(r"\bint dv_field_set_detect_objects\(dv_field_set\* set, int32_t on, int32_t segmap_on\);", header)
    assert re.search(r"\bint dv_field_set_detect_objects_read\(dv_field_set\* set, int64_t n_expected, "
                     r"const dv_detect_objects\* out\);", header)
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports) and re.search(r"local:\s*\*;", exports)
    for name in ("dv_scene_detect_objects", "dv_field_set_detect_objects", "dv_field_set_detect_objects_read"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    multi, obj = _lib.SIGNATURES["dv_scene_detect_multiband"][1], _lib.SIGNATURES["dv_scene_detect_objects"]
    # ctx fields M H W nb params cap n_out offsets globalrms and the seven catalogue arrays, as the multi-band call has them
    assert obj[0] is C.c_int and obj[1][:18] == multi[:18]
    assert obj[1][18:] == [C.POINTER(_lib.DvDetectWeights), C.POINTER(_lib.DvDetectBands), C.POINTER(_lib.DvDetectObjects)]
    assert _lib.SIGNATURES["dv_field_set_detect_objects"][1] == [C.c_void_p, C.c_int32, C.c_int32]
    assert _lib.SIGNATURES["dv_field_set_detect_objects_read"][1] == [C.c_void_p, C.c_int64, C.POINTER(_lib.DvDetectObjects)]
    assert _lib.SIGNATURES["dv_field_set_detect"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(_lib.DvDetectParams),
                                                                C.c_int64] + _lib.SIGNATURES["dv_field_set_detect"][1][4:])
    assert len(_lib.SIGNATURES["dv_field_set_detect"][1]) == 14
    # refused by the library itself on null handles, without a GPU
    assert _lib.lib.dv_field_set_detect_objects(None, 1, 1) == -1
    assert _lib.lib.dv_field_set_detect_objects_read(None, 0, None) == -1
    assert _lib.lib.dv_scene_detect_objects(*[0 if a in (C.c_int32, C.c_int64) else None for a in obj[1]]) == -1
