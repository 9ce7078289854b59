"""CPU checks of the detector's cleaning pass: the numpy restatement (tests/detect_clean_oracle.py) on
painted fields - the motivating case at three clean_param, a chain, an exact tie, the same coordinates in another field, every
column of a merged row, a field without absorption - each behind its premises; then the host layer on stand-ins: the columns
and their types, clean= through **kw, every ValueError before the library, detect_clean in iterative_catalogue, the header,
the export map and ctypes, the parameter lists.  No GPU is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import detect_clean_oracle as co
from tests import detect_objects_oracle as oo
from tests import stub_detect_clean_engine as stub
from tests import test_iterative_batch_host as bh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts_match(res):
    n = len(res["npix"])
    assert np.array_equal(np.bincount(res["segmap"].ravel(), minlength=n + 1)[1:], res["npix"])
    assert res["nmerged"].sum() == res["n_raw"] and res["npix"].sum() == res["raw"]["npix"].sum()


def test_motivating_case_near_blob_absorbed_far_blob_survives():
    data = co.motivating()
    mesas, far, near = 0, 1, 2                              # catalogue order: by first pixel
    seen = {}
    for beta in (0.5, 1.0, 2.0):
        exp, obj, res = co.painted(data, clean_param=beta)
        assert exp["npix"].tolist() == [441, 4, 4] and res["n_raw"] == 3
        assert obj["x_iso"][far] < obj["x_iso"][mesas] < obj["x_iso"][near]
        assert res["mthresh_raw"].tolist() == [6.25, 0.25, 0.25]
        co.check_premises(res, absorbed=beta < 2.0, survivor_in_zone=beta >= 1.0)
        seen[beta] = (res["tables"]["P"][near, mesas], res["tables"]["P"][far, mesas], res["root"].tolist())
        _counts_match(res)
    # the figures the case was designed with, to three digits
    for beta, p_near, p_far in ((0.5, 0.457, 0.349), (1.0, 0.292, 0.174), (2.0, 0.153, 0.059)):
        assert abs(seen[beta][0] - p_near) < 1e-3 and abs(seen[beta][1] - p_far) < 1e-3, (beta, seen[beta])
    assert seen[0.5][2] == [0, 0, 0]                        # both absorbed
    assert seen[1.0][2] == [0, 1, 0]                        # the near blob absorbed, the far one survives
    assert seen[2.0][2] == [0, 1, 2]                        # both survive


def test_chain_ends_in_its_root():
    exp, obj, res = co.painted(co.chain())
    co.check_premises(res, absorbed=True, survivor_in_zone=False)
    assert res["absorber"].tolist() == [0, 0, 1]            # C goes to B, B goes to A
    assert res["root"].tolist() == [0, 0, 0] and res["nmerged"].tolist() == [3]
    P = res["tables"]["P"]
    assert P[2, 0] < 0.25 < P[2, 1]                         # A alone would not have taken C
    assert res["npix"].tolist() == [441 + 49 + 4]
    _counts_match(res)


def test_exact_tie_goes_to_the_smaller_row():
    exp, obj, res = co.painted(co.tie(), clean_param=0.5)
    co.check_premises(res, absorbed=True, survivor_in_zone=False)
    assert obj["dflux"][0] == obj["dflux"][1]
    P = res["tables"]["P"]
    assert P[0, 1] == P[1, 0] > 0.25                        # each one's wings explain the other
    assert res["tables"]["zone"].tolist() == [[False, False], [True, False]]
    assert res["root"].tolist() == [0, 0] and res["survivors"].tolist() == [0]
    # the peak of the merged row: equal values, the earlier raw row
    assert (res["xpeak"][0], res["ypeak"][0]) == (obj["xpeak"][0], obj["ypeak"][0])
    _counts_match(res)


def test_same_coordinates_in_another_field_absorb_nothing():
    both = co.painted(co.motivating(far=False))[2]
    assert both["root"].tolist() == [0, 0]
    for part in (dict(near=False, far=False), dict(mesas=False, far=False)):          # the mesas alone; the near blob alone
        exp, obj, res = co.painted(co.motivating(**part))
        assert res["n_raw"] == 1 and res["root"].tolist() == [0] and res["nmerged"].tolist() == [1]
        assert not (res["flag"] & co.MERGED).any()


def test_every_column_of_a_merged_row():
    d = co.motivating()
    d[49, 80] = 9.0                                         # the near blob's brightest pixel: above the mesas' 7
    exp, obj, res = co.painted(d)
    co.check_premises(res)
    raw = res["raw"]
    assert res["root"].tolist() == [0, 1, 0] and res["survivors"].tolist() == [0, 1]
    k, s, v = 0, 0, 2                                       # the merged row, its survivor, its victim
    assert res["npix"][k] == raw["npix"][s] + raw["npix"][v] and res["nmerged"].tolist() == [2, 1]
    assert res["flux"][k] == raw["flux"][s] + raw["flux"][v] and res["dflux"][k] == raw["dflux"][s] + raw["dflux"][v]
    assert res["peak"][k] == 9.0 and (res["xpeak"][k], res["ypeak"][k]) == (80, 49)
    assert res["vpeak"][k] == 9.0 and (res["xvpeak"][k], res["yvpeak"][k]) == (80, 49)
    assert (res["xmin"][k], res["xmax"][k]) == (raw["xmin"][s], raw["xmax"][v])
    assert (res["ymin"][k], res["ymax"][k]) == (raw["ymin"][s], raw["ymax"][s])
    assert res["flag"][k] == raw["flag"][s] | raw["flag"][v] | co.MERGED == 16
    for name in ("x", "y", "x_iso", "y_iso", "x2", "y2", "xy", "parent"):
        assert res[name][k] == raw[name][s], name
    assert res["mthresh"].tolist() == [6.25, 0.25]
    # the survivor that absorbed nothing: its own bits, no new bit
    for name in co.SHARED:
        assert res[name][1] == raw[name][1], name
    assert res["segmap"][49, 80] == 1 and set(np.unique(res["segmap"])) == {0, 1, 2}
    assert ((res["segmap"] > 0) == (obj["segmap"] > 0)).all()
    _counts_match(res)


def test_field_without_absorption_keeps_every_column():
    exp, obj, res = co.painted(co.motivating(near=False))
    co.check_premises(res, absorbed=False, survivor_in_zone=True)
    assert res["root"].tolist() == [0, 1]
    for name in co.SHARED:
        assert np.array_equal(res[name], res["raw"][name]) and res[name].dtype == res["raw"][name].dtype, name
    assert np.array_equal(res["segmap"], obj["segmap"]) and res["nmerged"].tolist() == [1, 1]


def test_mthresh_counts_ties_and_short_objects():
    D = np.zeros((6, 8))
    D[1, 1:6] = [5.0, 3.0, 3.0, 3.0, 2.0]
    D[4, 1:3] = [4.0, 2.0]
    seg = np.zeros((6, 8), np.int32)
    seg[1, 1:6] = 1
    seg[4, 1:3] = 2
    for minarea, want in ((1, [4.0, 3.0]), (2, [2.0, 1.0]), (3, [2.0, 0.0]), (4, [2.0, 0.0]), (5, [1.0, 0.0]), (6, [0.0, 0.0])):
        assert co.mthresh(seg, D, 1.0, 2, minarea).tolist() == want, minarea


def test_crowded_scene_of_the_gpu_tests_holds_its_premises():
    """what tests/test_gpu_detect_clean.py asserts first, on the restatement alone"""
    exp, obj, res = co.painted(co.crowd(), minarea=1)
    co.check_premises(res)
    assert obj["npix"].max() > 2048 and res["n_raw"] > 256 and res["nmerged"].max() > 257
    assert (np.diff(res["survivors"]) > 0).all()
    _counts_match(res)


# ---- the host layer ------------------------------------------------------------------------------------------------------
def test_extract_objects_clean_columns_and_routing():
    from debvader_amd.detect import detection

    dt, cdt = detection.object_dtype(), detection.clean_object_dtype()
    assert list(cdt.names) == list(dt.names) + ["nmerged", "mthresh"]
    assert cdt["nmerged"] == np.int32 and cdt["mthresh"] == np.float64 and all(cdt[k] == dt[k] for k in dt.names)
    img = np.zeros((2, 8, 9, 3))
    ctx = stub.RecordingContext()
    # off by default: the call it always was
    recs = detection.extract_objects_batch(img, ctx=ctx, thresh=2.0)
    assert ctx.called == "scene_detect_objects" and ctx.kw == dict(segmentation_map=False, thresh=2.0)
    assert all(r.dtype == dt for r in recs)
    detection.extract_objects_batch(img, ctx=ctx, clean=False, clean_param=3.0)
    assert ctx.called == "scene_detect_objects" and ctx.kw == dict(segmentation_map=False)
    # on: popped from kw, handed on as clean_param
    recs = detection.extract_objects_batch(img, ctx=ctx, clean=True, thresh=2.0)
    assert ctx.called == "scene_detect_clean" and ctx.kw == dict(segmentation_map=False, thresh=2.0, clean_param=1.0)
    assert [len(r) for r in recs] == [2, 1] and all(isinstance(r, np.recarray) and r.dtype == cdt for r in recs)
    assert np.concatenate([r["nmerged"] for r in recs]).tolist() == [3, 1, 2]
    assert np.concatenate([r["mthresh"] for r in recs]).tolist() == [0.25, 0.5, 0.75]
    rec, seg = detection.extract_objects(img, ctx=ctx, segmentation_map=True, clean=True, clean_param=2.5)
    assert ctx.called == "scene_detect_clean" and ctx.kw["clean_param"] == 2.5 and ctx.shape == (1, 8, 9)
    assert rec.dtype == cdt and seg.shape == (8, 9)
    detection.extract_objects(img, ctx=ctx, bands=[0, 2], clean=True, weights=np.ones((2, 8, 9, 3)))
    assert ctx.called == "scene_detect_clean" and ctx.shape == (1, 8, 9, 3) and ctx.kw["weights"].shape == (1, 8, 9, 2)
    # detect_objects: the catalogue alone
    out = detection.detect_objects_batch(img, ctx=ctx, thresh=2.0)
    assert ctx.called == "scene_detect" and ctx.kw == dict(thresh=2.0) and len(out) == 2
    out = detection.detect_objects_batch(img, ctx=ctx, clean=True, thresh=2.0)
    assert ctx.called == "scene_detect_clean" and ctx.kw == dict(columns=False, clean_param=1.0, thresh=2.0)
    assert [len(o) for o in out] == [2, 1]
    d = detection.detect_objects(img, ctx=ctx, clean=True, clean_param=0.5)
    assert ctx.called == "scene_detect_clean" and ctx.kw == dict(columns=False, clean_param=0.5) and d.shape == (3, 2)
    detection.detect_objects(img, ctx=ctx)
    assert ctx.called == "scene_detect" and ctx.kw == {}
    detection.detect_objects(img, ctx=ctx, bands=None, clean=True)
    assert ctx.called == "scene_detect_clean" and ctx.kw["columns"] is False and ctx.shape == (1, 8, 9, 3)
    detection.detect_objects(img, ctx=ctx, bands=None)
    assert ctx.called == "scene_detect_multiband"
    for name in ("detect_objects", "detect_objects_batch", "extract_objects", "extract_objects_batch"):
        assert "sep" in getattr(detection, name).__doc__ and "clean" in getattr(detection, name).__doc__, name


def test_python_refusals_come_before_the_library():
    from debvader_amd import engine as E
    from debvader_amd.detect import detection

    f = np.zeros((1, 8, 9))
    call = E.Context.scene_detect_clean
    for bad in (dict(clean_param=0.0), dict(clean_param=-1.0), dict(clean_param=np.nan), dict(clean_param=np.inf),
                dict(clean_param=None), dict(clean_param="x"), dict(clean_param=True), dict(thresh=0.0), dict(thresh=-0.5),
                dict(thresh=np.nan), dict(minarea=65), dict(minarea=0), dict(bands=[0]), dict(noise="absolute"),
                dict(weights=np.ones((1, 8, 8))), dict(back_size=65)):
        with pytest.raises(ValueError):
            call(None, f, **bad)                              # (self is not reached)
    f4 = np.zeros((1, 8, 9, 3))
    for bad in (dict(thresh=0.0), dict(bands=[3]), dict(clean_param=0.0), dict(minarea=65)):
        with pytest.raises(ValueError):
            call(None, f4, **bad)
    with pytest.raises(ValueError, match="clean_param"):
        E.check_detect_clean(0.0, 1.5, 4)
    with pytest.raises(ValueError, match="thresh"):
        E.check_detect_clean(1.0, 0.0, 4)
    with pytest.raises(ValueError, match="minarea"):
        E.check_detect_clean(1.0, 1.5, 65)
    E.check_detect_clean(1.0, 1.5, 64)

    class Untouchable:                                        # a context that must not be reached
        def __getattr__(self, name):
            raise AssertionError(name)

    img = np.zeros((1, 8, 9, 3))
    for fn in (detection.detect_objects, detection.detect_objects_batch, detection.extract_objects,
               detection.extract_objects_batch):
        for bad in (dict(clean=True, clean_param=0.0), dict(clean=True, clean_param=np.nan), dict(clean=1.0),
                    dict(clean="yes"), dict(clean_param=-2.0)):
            with pytest.raises(ValueError):
                fn(img, ctx=Untouchable(), **bad)

    class Handle:                                             # a FieldSet whose handle must not be used
        shape = (1, 8, 8, 3)
        _detect_clean = True

        def _handle(self):
            return None

    with pytest.raises(ValueError, match="> 0"):
        E.FieldSet.detect(Handle(), thresh=0.0)
    with pytest.raises(ValueError, match="minarea"):
        E.FieldSet.detect(Handle(), minarea=65)

    class NoLibrary(Handle):
        def _handle(self):
            raise AssertionError("the library must not be reached")

    for bad in (0.0, -1.0, np.nan, "x"):
        with pytest.raises(ValueError, match="clean_param"):
            E.FieldSet.set_detect_clean(NoLibrary(), True, bad)


def test_parameter_lists():
    from debvader_amd import engine as E
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch
    from debvader_amd.detect import detection

    par = lambda f: list(inspect.signature(f).parameters)        # noqa: E731
    objects = par(E.Context.scene_detect_objects)
    assert par(E.Context.scene_detect_clean) == objects + ["clean_param"]
    assert inspect.signature(E.Context.scene_detect_clean).parameters["clean_param"].default == 1.0
    assert objects[-2:] == ["segmentation_map", "columns"] and "clean_param" not in objects
    sig = inspect.signature(E.FieldSet.set_detect_clean).parameters
    assert list(sig) == ["self", "on", "clean_param"] and sig["on"].default is True and sig["clean_param"].default == 1.0
    assert par(E.FieldSet.detect) == ["self", "active", "thresh", "minarea", "nthresh", "cont", "filter_kernel", "back_size",
                                      "back_filter", "workspace_bytes"]
    assert par(detection.detect_objects) == ["field_image", "ctx", "bands", "band_weights", "kw"]
    assert par(detection.detect_objects_batch) == ["field_images", "ctx", "bands", "band_weights", "kw"]
    assert par(detection.extract_objects) == ["field_image", "ctx", "bands", "band_weights", "segmentation_map", "kw"]
    assert par(detection.extract_objects_batch) == ["field_images", "ctx", "bands", "band_weights", "segmentation_map", "kw"]
    names = par(IterativeDeblendFieldBatch.iterative_catalogue)
    at = names.index("detect_clean")
    assert names[at - 1] == "detect_band_weights" and names[at + 1] == "detect_weights" and names[-1] == "fit_groups"
    assert inspect.signature(IterativeDeblendFieldBatch.iterative_catalogue).parameters["detect_clean"].default is None


def test_iterative_catalogue_with_detect_clean():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    script = [[(3, 1), (4, 0), (2, 0)], [(2, 2), (1, 0)]]
    plain, ref, core = bh._run(script)
    det_names = [n for n, _ in IterativeDeblendFieldBatch.DETECT_COLUMNS]
    for arg, beta in ((True, 1.0), (2.5, 2.5), (1, 1.0)):
        obj, eng = stub.batch(script)
        res = obj.iterative_catalogue(detect_clean=arg)
        names = [c[0] for c in eng.calls]
        assert names.count("set_detect_clean") == 1 and eng.calls[names.index("set_detect_clean")][1:] == (True, beta)
        assert names.index("open") < names.index("set_detect_clean") < names.index("detect")
        assert "set_detect_objects" not in names
        assert [c for c in names if c != "set_detect_clean"] == [c[0] for c in core.engine.calls]
        for a, b in zip(res, ref):                            # without detect_shapes: the columns of the plain run
            assert list(a.dtype.names) == list(b.dtype.names) and len(a) == len(b)
    # with detect_shapes: det_nmerged behind det_flag, the row's own
    obj, eng = stub.batch(script)
    res = obj.iterative_catalogue(detect_clean=True, detect_shapes=True)
    names = [c[0] for c in eng.calls]
    assert names.index("set_detect_objects") < names.index("set_detect_clean") < names.index("detect")
    for m, (a, b) in enumerate(zip(res, ref)):
        assert list(a.dtype.names) == list(b.dtype.names) + det_names + ["det_nmerged"]
        assert a["det_nmerged"].dtype == np.int32
        at = 0
        for k, (valid, invalid) in enumerate(script[m]):
            before = sum(sum(script[f][k]) for f in range(m) if k < len(script[f]))
            total = sum(sum(script[f][k]) for f in range(len(script)) if k < len(script[f]))
            np.testing.assert_array_equal(a["det_nmerged"][at:at + valid],
                                          stub.scripted_nmerged(k, total)[before + np.arange(valid)])
            at += valid
    # None and False: the calls of the loop as it was
    for arg in (None, False):
        obj, eng = stub.batch(script)
        obj.iterative_catalogue(detect_clean=arg)
        assert [c[0] for c in eng.calls] == [c[0] for c in core.engine.calls]
    # detect_shapes alone keeps its sixteen columns
    obj, eng = stub.batch(script)
    assert list(obj.iterative_catalogue(detect_shapes=True)[0].dtype.names)[-16:] == det_names
    # refused before the set is opened
    for bad in (dict(detect_clean=0.0), dict(detect_clean=-1.0), dict(detect_clean=np.nan), dict(detect_clean="x"),
                dict(detect_clean=True, detect_thresh=0.0)):
        obj, eng = stub.batch(script)
        with pytest.raises(ValueError):
            obj.iterative_catalogue(**bad)
        assert eng.calls == []


def test_header_export_map_and_ctypes_signatures():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    m = re.search(r"typedef struct dv_detect_clean \{([^}]*)\} dv_detect_clean;", header)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1))
    fields = [tuple(decl.replace("*", " ").split()) for decl in body.split(";") if decl.strip()]
    assert fields == [("double", "clean_param"), ("int32_t", "nmerged"), ("double", "mthresh"), ("int64_t", "n_raw")]
    assert [d.count("*") for d in body.split(";") if d.strip()] == [0, 1, 1, 1]
    assert _lib.DvDetectClean._fields_ == [("clean_param", C.c_double), ("nmerged", C.POINTER(C.c_int32)),
                                           ("mthresh", C.POINTER(C.c_double)), ("n_raw", C.POINTER(C.c_int64))]
    assert C.sizeof(_lib.DvDetectClean) == 32
    assert re.search(r"#define DV_DETECT_FLAG_MERGED 16\b", header) and _lib.DETECT_FLAG_MERGED == 16 == co.MERGED
    assert _lib.DETECT_CLEAN_MINAREA_MAX == 64
    m = re.search(r"\bint dv_scene_detect_clean\(dv_ctx\* ctx,([^;]*)\);", header)
    o = re.search(r"\bint dv_scene_detect_objects\(dv_ctx\* ctx,([^;]*)\);", header)
    norm = lambda s: re.sub(r"\s+", " ", s.strip())              # noqa: E731
    assert m and o and norm(m.group(1)) == norm(o.group(1)) + ", const dv_detect_clean* clean"
    assert re.search(r"\bint dv_field_set_detect_clean\(dv_field_set\* set, int32_t on, double clean_param\);", header)
    assert re.search(r"\bint dv_field_set_detect_clean_read\(dv_field_set\* set, int64_t n_expected, int32_t\* nmerged, "
                     r"double\* mthresh, int64_t\* n_raw\);", header)
    # the existing structs and entry points are as they were
    assert re.search(r"\bint dv_field_set_detect\(dv_field_set\* set, const uint8_t\* active, const dv_detect_params\* params, "
                     r"int64_t cap,", header)
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports) and re.search(r"local:\s*\*;", exports)
    for name in ("dv_scene_detect_clean", "dv_field_set_detect_clean", "dv_field_set_detect_clean_read"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    obj, cl = _lib.SIGNATURES["dv_scene_detect_objects"], _lib.SIGNATURES["dv_scene_detect_clean"]
    assert cl[0] is C.c_int and cl[1] == obj[1] + [C.POINTER(_lib.DvDetectClean)]
    assert _lib.SIGNATURES["dv_field_set_detect_clean"][1] == [C.c_void_p, C.c_int32, C.c_double]
    assert _lib.SIGNATURES["dv_field_set_detect_clean_read"][1] == [C.c_void_p, C.c_int64, C.POINTER(C.c_int32),
                                                                    C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    assert len(_lib.SIGNATURES["dv_field_set_detect"][1]) == 14
    # refused by the library itself on null handles, without a GPU
    assert _lib.lib.dv_field_set_detect_clean(None, 1, 1.0) == -1
    assert _lib.lib.dv_field_set_detect_clean_read(None, 0, None, None, None) == -1
    assert _lib.lib.dv_scene_detect_clean(*[0 if a in (C.c_int32, C.c_int64) else None for a in cl[1]]) == -1
    # the new translation unit is part of the build
    make = open(os.path.join(ROOT, "debvader_amd", "csrc", "Makefile")).read()
    assert "detect_clean.hip" in make
