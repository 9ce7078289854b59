"""The detector's cleaning pass on the GPU (Context.scene_detect_clean, dv_scene_detect_clean, FieldSet.set_detect_clean,
iterative_catalogue(detect_clean=)) against its numpy restatement (tests/detect_clean_oracle.py): on
painted fields of the weighted path, where every value is exact, on the noise scenes of the three paths at the first seed whose
premises hold, across the chunks of a batch, through the resident set and the iterative loop.  Every scene first passes its
premises on the restatement alone.  The fraction of every bound met is printed (DESIGN.md quotes the worst)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from tests import detect_clean_oracle as co
from tests import detect_objects_oracle as oo

pytestmark = pytest.mark.gpu

CAT = ("field", "parent", "npix", "peak", "flux", "x", "y")
INT = oo.INT_KEYS
DBL = oo.DOUBLE_KEYS
DERIVED = ("a", "b", "theta", "cxx", "cyy", "cxy")
ROWS = CAT[1:] + INT + DBL + DERIVED                        # what scene_detect_clean shares with scene_detect_objects
CLEAN = ("nmerged", "mthresh")
EXACT = ("npix", "parent") + INT                            # boxes, peak pixels, flag
H, W = 125, 157


def _ctx():
    from debvader_amd import engine as E
    return E.default_context()


def _same_bits(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype, k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _compare(got, i, res, raw, D, T, minarea):
    """field i of a scene_detect_clean result with a segmap against the restatement `res` of that field; raw: the result of
    scene_detect_objects on the same input (with its segmap), D the thresholded map of the call and T the field's threshold,
    whose bits mthresh has"""
    lo, hi = got["offsets"][i], got["offsets"][i + 1]
    rlo, rhi = raw["offsets"][i], raw["offsets"][i + 1]
    assert got["n_raw"][i] == res["n_raw"] == rhi - rlo
    assert hi - lo == len(res["survivors"])
    np.testing.assert_array_equal(got["nmerged"][lo:hi], res["nmerged"])
    np.testing.assert_array_equal(got["segmap"][i], res["segmap"])
    assert np.array_equal(np.bincount(got["segmap"][i].ravel(), minlength=hi - lo + 1)[1:], got["npix"][lo:hi])
    for k in EXACT:
        np.testing.assert_array_equal(got[k][lo:hi], res[k], err_msg=k)
    assert (got["field"][lo:hi] == i).all()
    # mthresh: the bits of the call's own D - T, at the minarea-th largest pixel of the raw object
    mine = co.mthresh(raw["segmap"][i], D, T, rhi - rlo, minarea)[res["survivors"]]
    np.testing.assert_array_equal(got["mthresh"][lo:hi], mine)
    np.testing.assert_allclose(got["mthresh"][lo:hi], res["mthresh"], rtol=0, atol=1e-12 * max(np.abs(D[np.isfinite(D)]).max(), 1.0))
    if hi == lo:
        return {}
    frac = {"flux": (np.abs(got["flux"][lo:hi] - res["flux"]) / (1e-12 * res["flux_abs"])).max(),
            "dflux": (np.abs(got["dflux"][lo:hi] - res["dflux"]) / (1e-12 * res["dflux_abs"])).max()}
    # the merge itself is sequential arithmetic on the raw rows: with the GPU's own raw rows every column has its bits
    s = rlo + res["survivors"]
    for k in ("x", "y", "x_iso", "y_iso", "x2", "y2", "xy"):
        np.testing.assert_array_equal(got[k][lo:hi], raw[k][s], err_msg=k)           # the survivor's own bits
    flux, dflux, peak, vpeak = (raw[k][s].copy() for k in ("flux", "dflux", "peak", "vpeak"))
    newrow = np.full(rhi - rlo, -1)
    newrow[res["survivors"]] = np.arange(hi - lo)
    for r in np.flatnonzero(res["root"] != np.arange(rhi - rlo)):
        k = newrow[res["root"][r]]
        flux[k] += raw["flux"][rlo + r]
        dflux[k] += raw["dflux"][rlo + r]
        peak[k] = max(peak[k], raw["peak"][rlo + r])
        vpeak[k] = max(vpeak[k], raw["vpeak"][rlo + r])
    for k, v in (("flux", flux), ("dflux", dflux), ("peak", peak), ("vpeak", vpeak)):
        np.testing.assert_array_equal(got[k][lo:hi], v, err_msg=k)
    print("fraction of the bound met:", ", ".join(f"{k} {f:.2e}" for k, f in frac.items()))
    for k, f in frac.items():
        assert f <= 1.0, (k, f)
    return frac


# ---- painted fields, the weighted path -------------------------------------------------------------------------------------
BATCH = ("crowd", "motivating", "lattice_alone", "zero")


@functools.lru_cache(maxsize=None)
def _painted_batch():
    """(fields (4, H, W), the restatement of each at minarea 1, clean_param 1): computed once, treat as read-only"""
    fields = np.stack([co.crowd(), co.motivating(H, W), co.lattice_alone(), np.zeros((H, W))])
    fields.setflags(write=False)
    return fields, [co.painted(f, minarea=1) for f in fields]


def _painted_kw(minarea):
    return dict(weights=None, minarea=minarea, **co.PAINTED_KW)


def _call(fields, minarea=1, clean_param=1.0, **kw):
    args = dict(_painted_kw(minarea), weights=np.ones_like(fields), segmentation_map=True, **kw)
    return _ctx().scene_detect_clean(fields, clean_param=clean_param, **args), args


def test_painted_batch_large_absorber_over_a_lattice():
    fields, ref = _painted_batch()
    exp, obj, res = ref[0]
    co.check_premises(res)                                     # the crowd: structure and margins
    assert obj["npix"].max() > 2048 and res["n_raw"] > 256 and res["nmerged"].max() > 257
    assert (obj["flag"] & oo.BLENDED).sum() == 25              # the comb: 25 objects of one component, in catalogue order
    co.check_premises(ref[1][2])                               # the motivating case at minarea 1
    assert ref[1][2]["root"].tolist() == [0, 1, 0]
    co.check_premises(ref[2][2], absorbed=False, survivor_in_zone=False)
    assert ref[2][2]["n_raw"] > 256 and (ref[2][2]["root"] == np.arange(ref[2][2]["n_raw"])).all()
    got, args = _call(fields)
    raw = _ctx().scene_detect_objects(fields, **args)
    assert got["n_raw"].tolist() == [r[2]["n_raw"] for r in ref] and got["n_raw"][3] == 0
    assert got["nmerged"].dtype == np.int32 and got["mthresh"].dtype == np.float64 and got["n_raw"].dtype == np.int64
    for i in range(4):
        _compare(got, i, ref[i][2], raw, fields[i], co.T_PAINTED, 1)
    # painted integers: every sum is exact, the restatement's columns are the GPU's
    for i in range(2):
        lo, hi = got["offsets"][i], got["offsets"][i + 1]
        for k in ("flux", "dflux", "peak", "vpeak", "mthresh"):
            np.testing.assert_array_equal(got[k][lo:hi], ref[i][2][k], err_msg=k)
    merged = got["nmerged"] > 1
    assert ((got["flag"] & 16) > 0).tolist() == merged.tolist() and merged.sum() == sum((r[2]["nmerged"] > 1).sum() for r in ref)
    # the field in which nothing is absorbed: the bits of scene_detect_objects in every shared output
    lo, hi = got["offsets"][2], got["offsets"][3]
    rlo, rhi = raw["offsets"][2], raw["offsets"][3]
    assert hi - lo == rhi - rlo > 256
    for k in ROWS:
        assert got[k].dtype == raw[k].dtype, k
        np.testing.assert_array_equal(got[k][lo:hi], raw[k][rlo:rhi], err_msg=k)
    np.testing.assert_array_equal(got["segmap"][2], raw["segmap"][2])
    np.testing.assert_array_equal(got["globalrms"], raw["globalrms"])
    assert (got["nmerged"][lo:hi] == 1).all()


def test_runs_do_not_see_order_batch_or_chunks():
    from debvader_amd._lib import DvError

    fields, ref = _painted_batch()
    a, args = _call(fields)
    keys = ROWS + CLEAN + ("field", "offsets", "globalrms", "segmap", "n_raw")
    _same_bits(a, _call(fields)[0], keys)                                              # a rerun
    with pytest.raises(DvError, match="workspace") as refused:
        _call(fields, workspace_bytes=1)
    need = int(re.search(r"needs up to (\d+) bytes", str(refused.value)).group(1))
    _same_bits(a, _call(fields, workspace_bytes=need)[0], keys)                        # one field per launch
    # the tables of the pass are counted only with the pass on
    with pytest.raises(DvError, match="workspace") as refused:
        _ctx().scene_detect_objects(fields, workspace_bytes=1, **args)
    plain = int(re.search(r"needs up to (\d+) bytes", str(refused.value)).group(1))
    assert need - plain == (H * W + 1) * (12 * 4 + 13 * 8) + 20
    r = _call(np.ascontiguousarray(fields[::-1]))[0]                                   # the fields reversed
    np.testing.assert_array_equal(r["segmap"][::-1], a["segmap"])
    np.testing.assert_array_equal(r["n_raw"][::-1], a["n_raw"])
    M = len(fields)
    for i in range(M):
        lo, hi = a["offsets"][i], a["offsets"][i + 1]
        rl, rh = r["offsets"][M - 1 - i], r["offsets"][M - i]
        one = _call(fields[i:i + 1])[0]                                                # each alone
        np.testing.assert_array_equal(one["segmap"][0], a["segmap"][i])
        assert one["n_raw"][0] == a["n_raw"][i]
        for k in ROWS + CLEAN:
            np.testing.assert_array_equal(r[k][rl:rh], a[k][lo:hi], err_msg=k)
            np.testing.assert_array_equal(one[k], a[k][lo:hi], err_msg=k)


def test_chain_tie_and_clean_param():
    Hs, Ws = 96, 120
    fields = np.stack([co.motivating(), co.chain(), co.tie()])
    for beta, roots in ((1.0, ([0, 1, 0], [0, 0, 0], [0, 1])), (0.5, ([0, 0, 0], [0, 0, 0], [0, 0])),
                        (2.0, ([0, 1, 2], [0, 1, 2], [0, 1]))):
        ref = [co.painted(f, minarea=4, clean_param=beta) for f in fields]
        for (exp, obj, res), want in zip(ref, roots):
            co.check_premises(res, absorbed=False, survivor_in_zone=False)
            assert res["root"].tolist() == want, (beta, res["root"])
        got, args = _call(fields, minarea=4, clean_param=beta)
        raw = _ctx().scene_detect_objects(fields, **args)
        for i in range(3):
            _compare(got, i, ref[i][2], raw, fields[i], co.T_PAINTED, 4)
    # the same coordinates in another field absorb nothing
    apart = np.stack([co.motivating(near=False, far=False), co.motivating(mesas=False, far=False)])
    got, args = _call(apart, minarea=4)
    assert got["n_raw"].tolist() == [1, 1] and got["nmerged"].tolist() == [1, 1] and not (got["flag"] & 16).any()
    _same_bits(got, _ctx().scene_detect_objects(apart, **args), ROWS + ("field", "offsets", "segmap"))
    assert (Hs, Ws) == fields.shape[1:]


# ---- the noise scenes of the three paths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["unweighted", "weighted", "multiband"])
def test_noise_scene(path):
    seed, fields, kw, exp, obj, res = co.first_noise_case(path)            # its premises hold, one companion is absorbed
    print(f"{path}: seed {seed}, {res['n_raw']} raw objects, nmerged {res['nmerged'].tolist()}")
    ctx = _ctx()
    call = dict(kw)
    if "weights" in call:
        call["weights"] = call["weights"][None]
    got = ctx.scene_detect_clean(fields[None], segmentation_map=True, **call)
    raw = ctx.scene_detect_objects(fields[None], segmentation_map=True, **call)
    if path == "multiband":
        maps = ctx.scene_detect_multiband(fields[None], return_maps=True, **call)
    else:
        maps = ctx.scene_detect(fields[None], return_maps=True, **call)
    T = 1.5 * maps["globalrms"][0] if path == "unweighted" else call["thresh"]
    frac = _compare(got, 0, res, raw, maps["D"][0], T, 4)
    assert frac and (got["nmerged"] > 1).sum() >= 1 and ((got["flag"] & 16) > 0).tolist() == (got["nmerged"] > 1).tolist()
    _same_bits(got, raw, ("globalrms",))
    d = oo.derived(got["x2"], got["y2"], got["xy"])
    for k in DERIVED:
        np.testing.assert_allclose(got[k], d[k], rtol=1e-13, atol=1e-13, err_msg=k)


# ---- the C ABI: a small cap, the catalogue alone, the refusals ---------------------------------------------------------------------
def _raw(fields, cap, objects=True, clean=True, clean_param=1.0, thresh=0.75, minarea=1, segmap=True):
    """dv_scene_detect_clean on painted fields with unit weights, through ctypes"""
    from debvader_amd import _lib
    from debvader_amd import engine as E

    M, Hf, Wf = fields.shape
    k1 = np.ones((1, 1))
    params = _lib.DvDetectParams(thresh, 1e-5, minarea, 64, 64, 3, E._dp(k1), 1, 1, 0)
    cat = {k: np.full(cap, -7, np.int32 if k in ("field", "parent", "npix") else np.float64) for k in CAT}
    arr = {k: np.full(cap, -7, np.int32 if k in INT else np.float64) for k in INT + DBL}
    if segmap:
        arr["segmap"] = np.full((M, Hf, Wf), -7, np.int32)
    ostruct = _lib.DvDetectObjects(**{k: (E._ip(v) if v.dtype == np.int32 else E._dp(v)) for k, v in arr.items()})
    cl = dict(nmerged=np.full(cap, -7, np.int32), mthresh=np.full(cap, -7.0), n_raw=np.full(M, -7, np.int64))
    cstruct = _lib.DvDetectClean(clean_param, E._ip(cl["nmerged"]), E._dp(cl["mthresh"]),
                                 cl["n_raw"].ctypes.data_as(C.POINTER(C.c_int64)))
    w = np.ones_like(fields)
    wstruct = _lib.DvDetectWeights(E._dp(w), 0, 0)
    n = C.c_int64(-1)
    offsets, grms = np.zeros(M + 1, np.int64), np.zeros(M)
    st = _lib.lib.dv_scene_detect_clean(
        _ctx()._h, E._dp(fields), M, Hf, Wf, 0, C.byref(params), cap, C.byref(n), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
        E._dp(grms), *[E._ip(cat[k]) if cat[k].dtype == np.int32 else E._dp(cat[k]) for k in CAT],
        C.byref(wstruct), None, C.byref(ostruct) if objects else None, C.byref(cstruct) if clean else None)
    return st, n.value, cat, arr, cl, offsets


def test_small_cap_catalogue_alone_and_refusals():
    from debvader_amd import _lib

    fields = np.ascontiguousarray(np.stack([co.motivating(), co.chain()]))
    kw = dict(_painted_kw(4), weights=np.ones_like(fields))
    before = _ctx().scene_detect_objects(fields, segmentation_map=True, **kw)
    full = _ctx().scene_detect_clean(fields, segmentation_map=True, **kw)
    assert len(full["x"]) == 3 and full["n_raw"].tolist() == [3, 3] and full["nmerged"].tolist() == [2, 1, 3]
    # a cap that is too small: n_out, n_raw and the segmap, no rows
    st, n, cat, arr, cl, off = _raw(fields, 2, minarea=4)
    assert st == 0 and n == 3 and cl["n_raw"].tolist() == [3, 3] and off.tolist() == [0, 2, 3]
    np.testing.assert_array_equal(arr["segmap"], full["segmap"])
    assert all((v == -7).all() for v in cat.values()) and all((arr[k] == -7).all() for k in INT + DBL)
    assert (cl["nmerged"] == -7).all() and (cl["mthresh"] == -7).all()
    st, n, cat, arr, cl, off = _raw(fields, 3, minarea=4)
    assert st == 0 and n == 3
    for k in CAT + INT + DBL + ("segmap",) + CLEAN:
        np.testing.assert_array_equal(arr[k] if k in arr else (cat[k] if k in cat else cl[k]), full[k], err_msg=k)
    # the catalogue alone: objects = NULL
    st, n, cat, arr, cl, off = _raw(fields, 8, objects=False, minarea=4)
    assert st == 0 and n == 3 and (arr["segmap"] == -7).all() and all((arr[k] == -7).all() for k in INT + DBL)
    for k in CAT:
        np.testing.assert_array_equal(cat[k][:3], full[k], err_msg=k)
        assert (cat[k][3:] == -7).all()
    assert cl["nmerged"][:3].tolist() == [2, 1, 3] and cl["n_raw"].tolist() == [3, 3]
    np.testing.assert_array_equal(cl["mthresh"][:3], full["mthresh"])
    alone = _ctx().scene_detect_clean(fields, columns=False, **kw)
    assert "segmap" not in alone and "x2" not in alone
    _same_bits(alone, full, CAT + CLEAN + ("offsets", "globalrms", "n_raw"))
    # each refusal, before any GPU work
    for bad, word in ((dict(clean=False), "clean request"), (dict(clean_param=0.0), "clean_param"),
                      (dict(clean_param=-1.0), "clean_param"), (dict(clean_param=np.nan), "clean_param"),
                      (dict(clean_param=np.inf), "clean_param"), (dict(thresh=0.0), "thresh"), (dict(thresh=-0.5), "thresh"),
                      (dict(minarea=65), "minarea"), (dict(minarea=0), "bad arguments")):
        st, n, cat, arr, cl, off = _raw(fields, 8, **bad)
        assert st == -1 and word in _lib.last_error(), (bad, _lib.last_error())
        assert n == -1 and (arr["segmap"] == -7).all() and (cl["n_raw"] == -7).all()
    sig = _lib.SIGNATURES["dv_scene_detect_clean"][1]
    null = [0 if a in (C.c_int32, C.c_int64) else None for a in sig]
    null[0] = _ctx()._h
    assert _lib.lib.dv_scene_detect_clean(*null) == -1
    assert _raw(fields, 8, minarea=64)[0] == 0                                         # the largest minarea the pass takes
    # the engine is as usable as before: an existing call gives the bits it gave
    after = _ctx().scene_detect_objects(fields, segmentation_map=True, **kw)
    _same_bits(before, after, ROWS + ("field", "offsets", "globalrms", "segmap"))


# ---- the resident set and the iterative loop --------------------------------------------------------------------------------------
def test_field_set_switch_on_and_off():
    from debvader_amd._lib import DvError
    from tests.test_gpu_fields_batch import _net

    net = _net("float32")
    ctx, eng = net._core.ctx, net._core.engine
    fields = co.loop_fields()
    band = np.ascontiguousarray(fields[:, :, :, 2])
    ref = ctx.scene_detect_clean(band, segmentation_map=True)
    assert ref["n_raw"].sum() > len(ref["x"]) > 0                                      # something is absorbed
    fs = eng.open_field_set(fields)
    old = fs.detect()
    shared = CAT + ("offsets", "globalrms")
    assert sorted(old) == sorted(shared)
    fs.set_detect_clean(True)
    got = fs.detect()
    assert set(got) == set(shared) | set(CLEAN) | {"n_raw"}
    _same_bits(ref, got, shared + CLEAN + ("n_raw",))
    assert len(got["x"]) < len(old["x"]) == ref["n_raw"].sum()
    # beside set_detect_objects: the cleaned columns and the cleaned segmap
    fs.set_detect_objects(True, segmentation_map=True)
    both = fs.detect()
    _same_bits(ref, both, shared + CLEAN + ("n_raw", "segmap") + ROWS)
    # a field that is not active: an empty range, n_raw 0
    part = fs.detect(active=np.array([False, True]))
    one = ctx.scene_detect_clean(band[1:], segmentation_map=True)
    assert part["n_raw"].tolist() == [0, one["n_raw"][0]] and part["offsets"].tolist() == [0, 0, len(one["x"])]
    _same_bits(one, part, ROWS + CLEAN)
    assert not part["segmap"][0].any()
    np.testing.assert_array_equal(part["segmap"][1], one["segmap"][0])
    # another clean_param; then held weights
    fs.set_detect_clean(True, 0.5)
    _same_bits(ctx.scene_detect_clean(band, segmentation_map=True, clean_param=0.5), fs.detect(), shared + CLEAN + ROWS + ("segmap",))
    w = np.full(band.shape, 1.0 / 0.05 ** 2)
    w[:, :, 66] = 0.0
    fs.set_detect_weights(w)
    fs.set_detect_clean(True)
    wref = ctx.scene_detect_clean(band, weights=w, back_size=32, segmentation_map=True)
    _same_bits(wref, fs.detect(back_size=32), shared + CLEAN + ROWS + ("segmap", "n_raw"))
    fs.set_detect_weights(None)
    with pytest.raises(ValueError):
        fs.detect(thresh=0.0)
    with pytest.raises(ValueError):
        fs.detect(minarea=65)
    # off again: the old keys, the old bits
    fs.set_detect_clean(False)
    fs.set_detect_objects(False)
    off = fs.detect()
    assert sorted(off) == sorted(shared)
    _same_bits(old, off, shared)
    from debvader_amd import _lib
    assert _lib.lib.dv_field_set_detect_clean_read(fs._h, len(off["x"]), None, None, None) == -1      # the switch is off
    fs.set_detect_clean(True)
    assert _lib.lib.dv_field_set_detect_clean_read(fs._h, len(off["x"]), None, None, None) == -1      # nothing kept yet
    n = len(fs.detect()["x"])
    assert _lib.lib.dv_field_set_detect_clean_read(fs._h, n + 1, None, None, None) == -1              # a wrong count
    assert _lib.lib.dv_field_set_detect_clean_read(fs._h, n, None, None, None) == 0
    assert _lib.lib.dv_field_set_detect_clean(fs._h, 1, 0.0) == -1 and "clean_param" in _lib.last_error()
    _same_bits(got, fs.detect(), shared + CLEAN)                                       # the refusal left the switch as it was
    fs.close()
    with pytest.raises(DvError, match="closed"):
        fs.set_detect_clean(True)


def test_iterative_catalogue_with_detect_clean():
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch
    from tests.test_gpu_fields_batch import CS, NB
    from tests.test_gpu_iterative_batch import _loop_net

    fields = co.loop_fields()
    for m in range(2):                                         # the scene is built for it: premises, and one absorbed per field
        exp, obj, details = oo.detect(fields[m, :, :, 2])
        oo.check_p3_p4(details)
        co.check_premises(co.clean(exp, obj, exp["D"], 1.5 * exp["globalrms"], 4, 1.0), survivor_in_zone=False)
    net = _loop_net("float32")

    def loop(**kw):
        net._core.seed_counter = 500
        it = IterativeDeblendFieldBatch(net, fields, CS, NB)
        return it, it.iterative_catalogue(max_iterations=1, detect_shapes=True, **kw)

    _, plain = loop()
    it, cleaned = loop(detect_clean=1.0)
    _, same = loop(detect_clean=True)
    ref = _ctx().scene_detect_clean(np.ascontiguousarray(fields[:, :, :, 2]))
    raw = _ctx().scene_detect_objects(np.ascontiguousarray(fields[:, :, :, 2]))
    det = [n for n, _ in IterativeDeblendFieldBatch.DETECT_COLUMNS]
    assert it.nb_of_detected_objects[0] == np.diff(ref["offsets"]).tolist()
    for m in range(2):
        a, b = plain[m], cleaned[m]
        assert list(b.dtype.names) == list(a.dtype.names) + ["det_nmerged"] and 0 < len(b) < len(a)
        assert ref["offsets"][m + 1] - ref["offsets"][m] < raw["offsets"][m + 1] - raw["offsets"][m]
        for name in b.dtype.names:
            assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(b[name], same[m][name])), name
        # the rows of the pass are the cleaned detections, selected by list_idx
        rows = ref["offsets"][m] + b["list_idx"]
        for name in det + ["det_nmerged"]:
            np.testing.assert_array_equal(b[name], ref[name[4:]][rows], err_msg=name)
        assert (b["det_nmerged"] > 1).sum() >= 1 and ((b["det_flag"] & 16) > 0).tolist() == (b["det_nmerged"] > 1).tolist()
        F = fields.shape[1]
        np.testing.assert_array_equal(b["galaxy_distances_to_center_y"], np.round(-int(F / 2) + b["det_x"]))
        np.testing.assert_array_equal(b["galaxy_distances_to_center_x"], np.round(-int(F / 2) + b["det_y"]))
        # a surviving row that absorbed nothing is the plain run's detection, column for column
        alone = np.flatnonzero(b["det_nmerged"] == 1)
        for j in alone:
            i = np.flatnonzero((a["det_x"] == b["det_x"][j]) & (a["det_y"] == b["det_y"][j]))
            assert len(i) == 1
            for name in det:
                assert a[name][i[0]] == b[name][j], name
