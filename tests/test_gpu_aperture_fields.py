"""The apertures on the fields on the GPU (dv_scene_aperture_fields, dv_infer_fields_measure_aper_data,
DeblendFieldBatch(apertures=..., aperture_data=True)).  Part 1: the stamp-free host call against the
numpy restatement of tests/aperture_fields_oracle.py.  Both sides start from the GPU's own catalogue and aperture rows
(dv_scene_measure, dv_scene_aperture), rho_auto included, so no decision can differ: the areas - sums of whole numbers - and
the NaN pattern are equal bit for bit, every sum lies within 1e-12 of the sum of its absolute terms (at most cs^2 = 3481
terms times 2^-53 is 4e-13 for any summation order), the model sums of a galaxy alone inside its field have the bits of
dv_scene_aperture's fluxes, and where the data field is a copy of the model field the two sums have the same bits.  Part 2:
the pipeline stage against the host call, bit for bit, on both engines, with fields, catalogue-only and with a field carried
across two groups.  The scene is that of tests/test_gpu_blend.py with one more galaxy, a stamp without a Kron radius."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import aperture_fields_oracle as afo
from tests import blend_oracle as bo
from tests.test_gpu_aperture import AP, CAT, COUNTS, CS, NB, _blob_fields, _net, _windows
from tests.test_gpu_blend import _scene as _blend_scene

pytestmark = pytest.mark.gpu

KEYS = afo.KEYS
RADII = {0: (), 3: (3.1, 5.3, 8.15), 8: (1.3, 2.45, 3.1, 4.15, 5.3, 6.45, 8.15, 11.3)}


def _ctx():
    from debvader_amd import engine as E

    return E.default_context()


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@functools.lru_cache(maxsize=None)
def _scene(cs, nb, F):
    """Five fields, 31 galaxies: (names, stamps float32, places, field_ptr, T, D, shape, status); never written to.  The 30
    galaxies of tests/test_gpu_blend.py - three alone in their field (inside, over a corner, at an edge), one field without
    stamps, a crowd with pairs, a triple, elliptical blobs, two stamps wholly outside, an all-zero stamp and an
    iteration-limit row - and, last in the crowd, "no kron": no light within 13 px (at 31 px) of the centre, measured with the
    row of the round pair galaxy before it, whose kron_limit ellipse it leaves empty."""
    names, stamps, places, fp, _, _ = _blend_scene(cs, nb, F)
    rr, cc = np.arange(cs, dtype=np.float64)[:, None], np.arange(cs, dtype=np.float64)[None, :]
    ctr, s = (cs - 1) / 2.0, cs / 31.0
    hole = np.where(np.hypot(rr - ctr, cc - ctr) > 13.0 * s, 0.4, 0.0)
    at = int(fp[4])                                                # behind the crowd of field 3
    names = names[:at] + ["no kron"] + names[at:]
    stamps = np.concatenate([stamps[:at], (hole[:, :, None] * np.ones(nb)).astype(np.float32)[None], stamps[at:]])
    c0 = (F - cs) // 2
    places = np.concatenate([places[:at], np.array([[c0 + 2, c0 - 3]], np.int32), places[at:]])
    fp = fp.copy()
    fp[4:] += 1
    cat = _ctx().scene_measure(stamps)
    shape, status = cat["shape"].copy(), cat["status"].copy()
    k = names.index("iteration limit")
    short = _ctx().scene_measure(stamps[k:k + 1], max_iter=3)
    shape[k], status[k] = short["shape"][0], short["status"][0]
    src = [i for i, n in enumerate(names) if n == "pair a"][1]
    shape[at], status[at] = shape[src], status[src]
    T = bo.composite(stamps, places, fp, 5, F)
    D = T + np.random.default_rng(77 + cs).normal(0.0, 0.05, size=T.shape)
    for a in (stamps, places, fp, T, D, shape, status):
        a.flags.writeable = False
    return names, stamps, places, fp, T, D, shape, status


@functools.lru_cache(maxsize=None)
def _aper(cs, nb, F, K, s):
    """dv_scene_aperture's rows of the scene"""
    _, stamps, _, _, _, _, shape, status = _scene(cs, nb, F)
    out = _ctx().scene_aperture(stamps, shape, status, None, radii=RADII[K], fractions=(), subsample=s)
    for a in out.values():
        a.flags.writeable = False
    return out


def _gpu(cs, nb, F, K, s, data=True, sel=None, fields=None, fp=None, D=None):
    _, _, places, fp0, T, D0, shape, status = _scene(cs, nb, F)
    ap = _aper(cs, nb, F, K, s)
    sel = slice(None) if sel is None else sel
    fields = slice(None) if fields is None else fields
    D = D0 if D is None else D
    return _ctx().scene_aperture_fields(shape[sel], status[sel], places[sel], ap["kron"][sel], ap["aper_status"][sel], T[fields],
                                        D[fields] if data else None, field_ptr=fp0 if fp is None else fp, cutout_size=cs,
                                        radii=RADII[K], subsample=s)


@pytest.mark.parametrize("cs,nb,F,K,s,data", [(31, 3, 64, 3, 5, True), (31, 3, 64, 8, 1, True), (31, 3, 64, 0, 5, False),
                                              (59, 6, 97, 3, 5, True), (59, 6, 97, 8, 5, False), (59, 6, 97, 0, 1, True)])
def test_scene_aperture_fields_against_the_restatement(cs, nb, F, K, s, data):
    names, stamps, places, fp, T, D, shape, status = _scene(cs, nb, F)
    ap = _aper(cs, nb, F, K, s)
    assert len(names) == 31 and np.diff(fp).tolist() == [1, 1, 0, 28, 1]
    ast = dict(zip(names, ap["aper_status"]))
    assert ast["zero"] == 4 and ast["no kron"] == 7 and status[names.index("iteration limit")] == 2 and ast["iteration limit"] == 0
    assert (np.abs(shape[[n == "elliptical" for n in names], 3]) > 0.1).all()
    par = afo.params(radii=RADII[K], subsample=s)
    ref = afo.aperture_fields(shape, status, ap["aper_status"], ap["kron"], places, fp, T, D if data else None, cs, par, True)
    got = _gpu(cs, nb, F, K, s, data)
    assert sorted(got) == sorted(KEYS) and got["ap_model_sum"].shape == (31, K, nb) and got["auto_field_area"].shape == (31,)
    worst = 0.0
    for i, (name, w) in enumerate(zip(names, ref)):
        for k in ("ap_field_area", "auto_field_area"):                           # whole numbers over s^2: bit for bit
            assert np.array_equal(got[k][i], w[k], equal_nan=True), (i, name, k)
        for k, a in (("ap_model_sum", "ap_model_abs"), ("auto_model_sum", "auto_model_abs"), ("ap_data_sum", "ap_data_abs"),
                     ("auto_data_sum", "auto_data_abs")):
            g, r = got[k][i], np.asarray(w[k])
            assert np.array_equal(np.isnan(g), np.isnan(r)), (i, name, k)
            fin = ~np.isnan(r)
            if fin.any():
                rel = np.abs(g[fin] - r[fin]) / np.where(w[a][fin] > 0, w[a][fin], 1.0)
                assert (np.abs(g[fin] - r[fin]) <= 1e-12 * w[a][fin]).all(), (i, name, k, rel.max())
                worst = max(worst, float(rel.max()))
        if not data:
            assert np.isnan(got["ap_data_sum"][i]).all() and np.isnan(got["auto_data_sum"][i]).all()
    print(f"{cs}/{nb}/K{K}/s{s}: sums within {worst:.1e} of the sums of their absolute terms")
    # the NaN pattern: the zero stamp has nothing, the stamp without Kron radius its circles
    z, h = names.index("zero"), names.index("no kron")
    assert all(np.isnan(got[k][z]).all() for k in KEYS)
    assert all(np.isnan(got[k][h]).all() for k in KEYS if k.startswith("auto_"))
    assert not np.isnan(got["ap_model_sum"][h]).any() and not np.isnan(got["ap_field_area"][h]).any()
    rest = [i for i in range(31) if i not in (z, h)]
    assert not any(np.isnan(got[k][rest]).any() for k in ("ap_model_sum", "ap_field_area", "auto_model_sum", "auto_field_area"))
    # wholly outside: nothing is summed
    for i in [i for i, n in enumerate(names) if n == "outside"]:
        assert all((got[k][i] == 0.0).all() for k in KEYS if data or not k.endswith("data_sum")), i
    # alone inside its field: T holds the widened stamp values, the sums are dv_scene_aperture's
    i = names.index("alone inside")
    assert np.array_equal(got["ap_model_sum"][i], ap["ap_flux"][i]) and np.array_equal(got["auto_model_sum"][i], ap["flux_auto"][i])
    assert np.array_equal(got["ap_field_area"][i], ap["ap_area"][i]) and got["auto_field_area"][i] == ap["kron"][i, 2]
    assert (got["auto_model_sum"][i] > 0).all()
    # over a corner and at an edge the field cuts the apertures
    for n in ("alone corner", "alone edge"):
        i = names.index(n)
        assert got["auto_field_area"][i] < ap["kron"][i, 2], n
        assert K == 0 or got["ap_field_area"][i, -1] < ap["ap_area"][i, -1], n
    crowd = [i for i, n in enumerate(names) if n in ("pair a", "pair b")]              # (inside the field: T >= P everywhere)
    assert (got["auto_model_sum"][crowd, 2] > ap["flux_auto"][crowd, 2]).all()


@pytest.mark.parametrize("cs,nb,F", [(31, 3, 64), (59, 6, 97)])
def test_rows_keep_their_bits(cs, nb, F):
    names, stamps, places, fp, T, D, shape, status = _scene(cs, nb, F)
    K, s = 3, 5
    got = _gpu(cs, nb, F, K, s)
    # the data field a copy of the model field: the two sums have the same bits on every row
    same = _gpu(cs, nb, F, K, s, D=T)
    assert _eq(same["ap_data_sum"], same["ap_model_sum"]) and _eq(same["auto_data_sum"], same["auto_model_sum"])
    for k in ("ap_model_sum", "ap_field_area", "auto_model_sum", "auto_field_area"):
        assert _eq(same[k], got[k]), k
    # without the data field the model sums keep their bits
    bare = _gpu(cs, nb, F, K, s, data=False)
    for k in ("ap_model_sum", "ap_field_area", "auto_model_sum", "auto_field_area"):
        assert _eq(bare[k], got[k]), k
    # the crowd shuffled within its field
    order = np.arange(31)
    order[fp[3]:fp[4]] = fp[3] + np.random.default_rng(1).permutation(int(fp[4] - fp[3]))
    shuffled = _gpu(cs, nb, F, K, s, sel=order)
    for k in KEYS:
        assert _eq(shuffled[k], got[k][order]), k
    # the fields in reverse order
    order = np.concatenate([np.arange(fp[m], fp[m + 1]) for m in range(4, -1, -1)])
    fp_r = np.concatenate([[0], np.cumsum(np.diff(fp)[::-1])])
    moved = _gpu(cs, nb, F, K, s, sel=order, fields=slice(None, None, -1), fp=fp_r)
    for k in KEYS:
        assert _eq(moved[k], got[k][order]), k
    # one galaxy of the crowd alone in the call
    for i in (5, names.index("no kron"), names.index("alone edge")):
        m = int(np.searchsorted(fp, i, side="right")) - 1
        one = _gpu(cs, nb, F, K, s, sel=slice(i, i + 1), fields=slice(m, m + 1), fp=np.array([0, 1]))
        for k in KEYS:
            assert _eq(one[k][0], got[k][i]), (i, k)


# ---- part 2: the pipeline -----------------------------------------------------------------------------------------------------
F2 = 131
KW = dict(radii=(2.0, 4.5), fractions=(0.3, 0.5, 0.9))


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_host_call(dtype, monkeypatch):
    from debvader_amd._lib import DvError

    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(5, F2, seed=11)
    starts, places, fp = _windows(F2, COUNTS, seed=5)
    seed = 77

    def reference(fields, starts, places, fp, **kw):
        rows = eng.infer_fields_measure_aper(fields, starts, fp, places=places, seed=seed, **kw)
        comp = eng.infer_fields_composite(fields, starts, places, fp, seed=seed)
        assert np.array_equal(rows["mean_fields"], comp["mean_fields"])
        want = ctx.scene_aperture_fields(rows["shape"], rows["status"], places, rows["kron"], rows["aper_status"],
                                         comp["mean_fields"], fields, field_ptr=fp, cutout_size=CS, radii=kw["radii"],
                                         subsample=kw.get("subsample", 5))
        return rows, want

    rows, want = reference(fields, starts, places, fp, **KW)
    ok = rows["aper_status"] == 0
    cut = ok & (want["auto_field_area"] != rows["kron"][:, 2])
    print(f"[{dtype}] aper_status {np.bincount(rows['aper_status'], minlength=8).tolist()}, the field cuts the Kron ellipse of "
          f"{int(cut.sum())} galaxies")
    assert ok.any()

    got = eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=seed, **KW)
    assert sorted(got) == sorted(tuple(rows) + KEYS)
    for k in KEYS:
        assert _eq(got[k], want[k]), k
    for k in rows:                                                # every shared output has infer_fields_measure_aper's bits
        assert _eq(got[k], rows[k]), k
    # catalogue-only: the mean field is composited on the device and stays there
    only = eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=seed, return_fields=False, **KW)
    assert sorted(only) == sorted(CAT + ("mse_center",) + AP + KEYS)
    for k in only:
        assert _eq(only[k], got[k]), k
    # grouped: three resident fields at a time, so field 2 (stamps 30 .. 179, chunks of 64) is carried from the first group
    # into the second and its field sums run there (tests/test_gpu_blend.py derives the limits: a field is 824 KB, 4 per
    # field with the result fields, 2 catalogue-only; one MiB less holds two fields and chunk 0 spans three)
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "9")
    with pytest.raises(DvError, match="come from 3 fields, device memory holds 2"):
        eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=seed, **KW)
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "10")
    grouped = eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=seed, **KW)
    for k in got:
        assert _eq(grouped[k], got[k]), k
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "4")
    with pytest.raises(DvError, match="come from 3 fields, device memory holds 2"):
        eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=seed, return_fields=False, **KW)
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "5")
    g2 = eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=seed, return_fields=False, **KW)
    for k in only:
        assert _eq(g2[k], only[k]), k
    # the blendedness call shares the device-side mean field: the bits of dv_scene_blend, as before
    stamps = eng.infer_fields(fields, starts, fp, seed=seed)["loc"]
    bl = ctx.scene_blend(stamps, rows["shape"], rows["status"], places, rows["mean_fields"], fields, field_ptr=fp)
    b = eng.infer_fields_measure_blend(fields, starts, fp, places, seed=seed, return_fields=False)     # (field 2 carried)
    assert _eq(b["blend"], bl["blend"]) and _eq(b["npix"], bl["npix"]) and _eq(b["shape"], rows["shape"])
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    for rf in (True, False):
        b = eng.infer_fields_measure_blend(fields, starts, fp, places, seed=seed, return_fields=rf)
        assert _eq(b["blend"], bl["blend"]) and _eq(b["npix"], bl["npix"]) and _eq(b["shape"], rows["shape"]), rf
    # other parameters reach the kernel, no radii; M = 1 is the single-field view
    kw0 = dict(radii=(), fractions=(), subsample=3, kron_factor=2.0, kron_min=2.5, kron_limit=5.0, band=0, max_iter=9)
    rows0, want0 = reference(fields, starts, places, fp, **kw0)
    b0 = eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=seed, return_fields=False, **kw0)
    assert all(_eq(b0[k], want0[k]) for k in KEYS) and b0["ap_model_sum"].shape == (len(starts), 0, NB)
    assert _eq(b0["kron"], rows0["kron"]) and not _eq(b0["auto_model_sum"], got["auto_model_sum"])
    m = 3
    s1, p1 = starts[fp[m]:fp[m + 1]], places[fp[m]:fp[m + 1]]
    fp1 = np.array([0, len(s1)], np.int64)
    rows1, want1 = reference(fields[m:m + 1], s1, p1, fp1, **KW)
    one = eng.infer_cutouts_measure_aper_data(fields[m], s1, p1, seed=seed, **KW)
    assert "mean_field" in one and np.array_equal(one["mean_field"], rows1["mean_fields"][0])
    assert all(_eq(one[k], want1[k]) for k in KEYS) and all(_eq(one[k], rows1[k]) for k in CAT + AP)


def test_deblend_field_batch_takes_the_apertures_on_the_fields():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    fields = _blob_fields(3, F2, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-45, 46, size=(n, 2)).astype(np.float64) for n in (20, 0, 45)]
    sky = np.linspace(0.03, 0.06, 3 * NB).reshape(3, NB)
    apertures = (3.0, 5.0, 8.0)

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds
        return DeblendFieldBatch(net, fields, CS, NB)

    a, b, c, d = batch(), batch(), batch(), batch()
    res = a.deblend_fields(dists, on_device=True, measure=True, apertures=apertures, aperture_data=True, sky_sigma=sky)
    plain = b.deblend_fields(dists, on_device=True, measure=True, apertures=apertures)
    host = c.deblend_fields(dists, measure=True)                  # the default path: stamps and catalogue on the host
    model = c.get_predicted_fields()["predicted_mean_fields"]
    assert np.array_equal(model, a.get_predicted_fields()["predicted_mean_fields"])
    names = tuple(n[0] for n in ms.aperture_data_dtype(NB, 3))
    want_cols = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) +
                         DeblendFieldBatch.aperture_columns(NB, 3, 3) + DeblendFieldBatch.aperture_data_columns(NB, 3))
    for m, (r, p, h) in enumerate(zip(res, plain, host)):
        assert r.dtype == want_cols and len(r) == len(p)
        for k in p.dtype.names:                                   # the columns of the call without it, value for value
            if k != "shifts":
                assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].base.kind == "f"), k
        if not len(r):
            continue
        mean = np.stack([np.asarray(x) for x in h["output_images_mean"]])
        stddev = np.stack([np.asarray(x) for x in h["output_images_stddev"]])
        places = int((F2 - CS) / 2) + dists[m].astype(np.int64)
        aps = ms.measure_apertures(mean, stddev, catalogue=h, radii=apertures, ctx=c._ctx)
        want = ms.measure_apertures_on_fields(h, places, model[m], fields[m], sky_sigma=sky[m], apertures=aps, radii=apertures,
                                              cutout_size=CS, ctx=c._ctx)
        for k in names:
            assert np.array_equal(r[k], want[k], equal_nan=True), (m, k)
        ok = r["aper_status"] == 0
        assert ok.sum() >= len(r) // 2 and np.isfinite(r["flux_auto_data"][ok]).all() and (r["flux_auto_data_err"][ok] > 0).all()
    cat = d.deblend_fields(dists, on_device=True, measure=True, apertures=apertures, aperture_data=True, sky_sigma=sky,
                           return_fields=False)
    for r, q in zip(res, cat):
        for k in r.dtype.names:
            if k != "shifts":
                assert np.array_equal(r[k], q[k], equal_nan=r.dtype[k].base.kind == "f"), k


def test_refusals_come_before_any_gpu_work_and_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import Engine, _dp, _ip, aperture_params

    DvError, lib = _lib.DvError, _lib.lib
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(1, F2, seed=11)
    starts, places, fp = _windows(F2, [5], seed=5, hang=False)
    good = eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=3)

    n, nb, K, J = 5, NB, 3, 3
    ptr = lambda a: None if a is None else (_dp(a) if a.dtype == np.float64 else _ip(a))     # noqa: E731
    cat = [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    ap = [np.zeros((n, K, nb)), np.zeros((n, K, nb)), np.zeros((n, K)), np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 3)),
          np.zeros((n, J)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    six = lambda n, nb: [np.zeros((n, K, nb)), np.zeros((n, K, nb)), np.zeros((n, K)), np.zeros((n, nb)), np.zeros((n, nb)),   # noqa: E731
                         np.zeros(n)]
    af = six(n, nb)
    f2, N, args = Engine._field_args(fields, starts, fp, places)
    mean_f, std_f, res_f = np.empty(f2.shape), np.empty(f2.shape), np.empty(f2.shape)

    def pipeline(par=None, apar=None, out=None, fields_out=(None, None, None), no_params=False, no_places=False, aper=None):
        par = par or _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
        apar = apar or aperture_params()
        a = list(args)
        if no_places:
            a[5] = None
        _lib.check(lib.dv_infer_fields_measure_aper_data(eng._h, *a, 9, C.byref(par), *fields_out, None, *map(ptr, cat),
                                                         None if no_params else C.byref(apar), *map(ptr, ap if aper is None else aper),
                                                         *map(ptr, af if out is None else out)))

    T = np.zeros((2, 40, 40, 3))
    sh, st, kr, pl = np.zeros((3, 5)), np.zeros(3, np.int32), np.zeros((3, 3)), np.zeros((3, 2), np.int32)
    af2 = six(3, 3)

    def scene(shape=sh, status=st, places=pl, fptr=(0, 2, 3), kron=kr, astatus=st, n=3, cs=31, nb=3, model=T, data=T, M=2, F=40,
              apar=None, out=None, no_params=False):
        apar = apar or aperture_params()
        fptr = None if fptr is None else np.asarray(fptr, np.int64)
        _lib.check(lib.dv_scene_aperture_fields(ctx._h, ptr(shape), ptr(status), ptr(places),
                                                None if fptr is None else fptr.ctypes.data_as(C.POINTER(C.c_int64)), ptr(kron),
                                                ptr(astatus), n, cs, nb, ptr(model), ptr(data), M, F,
                                                None if no_params else C.byref(apar), *map(ptr, af2 if out is None else out)))

    def edited(**kw):
        p = aperture_params()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, v[0])[v[1]] = v[2]
            else:
                setattr(p, k, v)
        return p

    nan = float("nan")
    for call in (pipeline, scene):
        with pytest.raises(DvError, match="params must be given"):
            call(no_params=True)
        for apar, msg in ((edited(n_radii=9), "0 .. 8 radii"), (edited(n_fractions=5), "0 .. 4 fractions"),
                          (edited(r=("radii", 1, 0.0)), "radius 1"), (edited(r=("radii", 2, nan)), "radius 2"),
                          (edited(f=("fractions", 0, 0.0)), "fraction 0"), (edited(subsample=0), "subsample"),
                          (edited(subsample=10), "subsample"), (edited(bisect_iters=0), "bisect_iters"),
                          (edited(kron_factor=0.0), "kron_factor"), (edited(kron_min=-1.0), "kron_min"),
                          (edited(kron_limit=nan), "kron_limit")):
            with pytest.raises(DvError, match=msg):
                call(apar=apar)
        for k in range(6):                                        # a missing output
            out = list(af if call is pipeline else af2)
            out[k] = None
            with pytest.raises(DvError, match="must all be given"):
                call(out=out)
    # the pipeline: a null places in both forms, a missing aperture output, what dv_infer_fields_measure refuses
    with pytest.raises(DvError, match="places"):
        pipeline(no_places=True)
    with pytest.raises(DvError, match="places"):
        pipeline(no_places=True, fields_out=(_dp(mean_f), _dp(std_f), None))
    for k in range(9):
        out = list(ap)
        out[k] = None
        with pytest.raises(DvError, match="must all be given|go together"):
            pipeline(aper=out)
    for par, msg in ((_lib.DvMeasureParams(NB, 3.0, 1e-10, 200), "band"), (_lib.DvMeasureParams(2, 0.0, 1e-10, 200), "sigma0"),
                     (_lib.DvMeasureParams(2, 3.0, 0.0, 200), "tol"), (_lib.DvMeasureParams(2, 3.0, 1e-10, -1), "max_iter")):
        with pytest.raises(DvError, match=msg):
            pipeline(par=par)
    with pytest.raises(DvError, match="go together"):
        pipeline(fields_out=(_dp(mean_f), None, None))
    # the host call: its inputs, the field table, the placements, the sizes
    for kw, msg in ((dict(shape=None), "must all be given"), (dict(status=None), "must all be given"),
                    (dict(places=None), "must all be given"), (dict(kron=None), "must all be given"),
                    (dict(astatus=None), "must all be given"), (dict(model=None), "must all be given"),
                    (dict(fptr=None), "must all be given"), (dict(fptr=(1, 2, 3)), "field_ptr must run from 0"),
                    (dict(fptr=(0, 2, 4)), "field_ptr must run from 0"), (dict(fptr=(0, 4, 3)), "decreases at field 1"),
                    (dict(fptr=(0, -1, 3)), "decreases at field 0"),
                    (dict(places=np.array([[0, 0], [1 << 29, 0], [0, 0]], np.int32)), "placement 1"),
                    (dict(places=np.array([[0, 0], [0, 0], [0, -(1 << 29)]], np.int32)), "placement 2"),
                    (dict(F=0), "fields of 0 pixels"), (dict(F=40000), "fields of 40000 pixels"),
                    (dict(cs=0), "stamps of 0 pixels"), (dict(cs=91), "at most 90 pixels"), (dict(nb=17), "17 bands"),
                    (dict(nb=0), "0 bands")):
        with pytest.raises(DvError, match=msg):
            scene(**kw)
    # without radii the circle outputs may be null; without data the call runs; nothing to do with N = 0
    none = list(af2)
    none[0] = none[1] = none[2] = None
    scene(apar=edited(n_radii=0), out=none)
    scene(data=None)
    assert np.isnan(af2[1]).all() and np.isnan(af2[4]).all()
    scene(n=0, fptr=(0, 0, 0), shape=None, status=None, places=None, kron=None, astatus=None, out=[None] * 6)
    # the engine completes a correct call afterwards, with the bits it gave before
    again = eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=3)
    for k in good:
        assert _eq(again[k], good[k]), k
    pipeline(fields_out=(_dp(mean_f), _dp(std_f), _dp(res_f)))
    assert np.array_equal(mean_f, eng.infer_fields_composite(fields, starts, places, fp, seed=9)["mean_fields"])
    ref = eng.infer_fields_measure_aper_data(fields, starts, fp, places, seed=9)
    assert _eq(ap[5], ref["kron"]) and all(_eq(a, ref[k]) for a, k in zip(af, KEYS))
