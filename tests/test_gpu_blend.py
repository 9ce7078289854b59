"""The blendedness sums on the GPU (dv_scene_blend, dv_infer_fields_measure_blend, DeblendFieldBatch(blendedness=True);
DESIGN.md section 7l).  Part 1: the stamp-level call against the numpy restatement of tests/blend_oracle.py - npix and the
NaN pattern equal on every row, every sum within 1e-12 sum g |x| of the restatement (at most 59^2 = 3481 terms times 2^-53 is
4e-13 for any summation order; the two evaluations of g differ by the few ulp of exp), A and Bm bit-equal for a galaxy alone
in its field.  Part 2: the pipeline stage against the stamp-level call, bit for bit, on both engines."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import blend_oracle as bo
from tests import measure_oracle as mo

pytestmark = pytest.mark.gpu


def _ctx():
    from debvader_amd import engine as E

    return E.default_context()


@functools.lru_cache(maxsize=None)
def _scene(cs, nb, F):
    """Five fields, 30 galaxies: (names, stamps float32, places, field_ptr, model fields T, data fields D); never written to.
    Field 0: one galaxy alone, inside.  Field 1: one alone, hanging over the top-left corner.  Field 2: no stamps.  Field 3:
    the crowd.  Field 4: one alone, clipped at the bottom-right edge."""
    rng = np.random.default_rng(1000 + cs)
    ctr = (cs - 1) / 2.0
    s = cs / 31.0                                                  # blob sizes follow the stamp
    gal = []                                                       # (name, field, plane, place)

    def blob(M, off=(0.0, 0.0), amp=1.0):
        return amp * mo.gaussian_stamp(cs, tuple(m * s * s for m in M), tuple(o * s for o in off))

    gal.append(("alone inside", 0, blob((5.0, 1.5, 7.0), (0.6, -0.4)), (F - cs - 3, 2)))
    gal.append(("alone corner", 1, blob((6.0, -2.0, 4.0), (-1.2, 0.9)), (-cs // 3, -cs // 4)))
    c0 = (F - cs) // 2
    crowd = [("isolated", blob((3.0, 0.0, 3.0)), (0, 0)), ("isolated", blob((2.5, 0.4, 4.0), (0.5, 0.5)), (F - cs, 0)),
             ("pair a", blob((4.0, 0.0, 4.0), amp=2.0), (c0, c0)), ("pair a", blob((4.0, 0.0, 4.0)), (c0, c0 + int(4 * s))),
             ("pair b", blob((6.0, 2.5, 5.0), (1.0, -1.0)), (3, F - cs - 2)),
             ("pair b", blob((3.0, -1.0, 8.0), (-2.0, 0.5), amp=0.5), (3 + int(6 * s), F - cs - 5)),
             ("triple", blob((4.0, 1.0, 4.0)), (F - cs - 1, F - cs - 1)),
             ("triple", blob((5.0, -1.5, 3.0), amp=1.5), (F - cs - 1 - int(3 * s), F - cs + 2)),
             ("triple", blob((3.5, 0.0, 6.0), amp=0.7), (F - cs + 1, F - cs - 1 - int(5 * s))),
             ("corner", blob((4.0, 1.2, 5.0), (2.0, 2.0)), (-int(9 * s), -int(11 * s))),
             ("outside", blob((4.0, 0.0, 4.0)), (-cs, 5)), ("outside", blob((4.0, 0.0, 4.0)), (7, F)),
             ("zero", np.zeros((cs, cs)), (c0, 2)), ("iteration limit", blob((7.0, 3.0, 6.0), (1.5, -2.5)), (c0 - 3, c0 + 5))]
    for k in range(13):                                            # elliptical blobs scattered over the field, Mrc != 0
        a, b = rng.uniform(2.0, 8.0, size=2)
        M = (a, rng.choice([-1.0, 1.0]) * rng.uniform(0.2, 0.7) * np.sqrt(a * b), b)
        crowd.append(("elliptical", blob(M, rng.uniform(-2.0, 2.0, size=2), rng.uniform(0.5, 3.0)),
                      tuple(rng.integers(-cs // 2, F - cs // 2, size=2))))
    gal += [(n, 3, p, pl) for n, p, pl in crowd]
    gal.append(("alone edge", 4, blob((5.0, 0.0, 5.0), (0.0, 1.0)), (F - cs // 2, F - 2 * cs // 3)))
    n = len(gal)
    stamps = np.zeros((n, cs, cs, nb), np.float32)
    for i, (name, _, p, _) in enumerate(gal):
        for b_ in range(nb):
            floor = 0.0 if name == "zero" else rng.uniform(0.0, 0.01, size=p.shape)
            stamps[i, :, :, b_] = (1.0 if b_ == 2 else rng.uniform(0.3, 2.0)) * p + floor
    places = np.array([g[3] for g in gal], np.int32)
    counts = np.bincount([g[1] for g in gal], minlength=5)
    fp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    T = bo.composite(stamps, places, fp, 5, F)
    D = T + rng.normal(0.0, 0.05, size=T.shape)
    for a in (stamps, places, fp, T, D):
        a.flags.writeable = False
    return [g[0] for g in gal], stamps, places, fp, T, D


@functools.lru_cache(maxsize=None)
def _rows(cs, nb, F):
    """The catalogue rows of the scene from dv_scene_measure; the "iteration limit" stamp measured with max_iter = 3"""
    names, stamps, *_ = _scene(cs, nb, F)
    cat = _ctx().scene_measure(stamps)
    k = names.index("iteration limit")
    short = _ctx().scene_measure(stamps[k:k + 1], max_iter=3)
    shape, status = cat["shape"].copy(), cat["status"].copy()
    shape[k], status[k] = short["shape"][0], short["status"][0]
    shape.flags.writeable = status.flags.writeable = False
    return shape, status


@pytest.mark.parametrize("cs,nb,F", [(31, 3, 64), (59, 6, 97)])
def test_scene_blend_against_the_restatement(cs, nb, F):
    names, stamps, places, fp, T, D = _scene(cs, nb, F)
    shape, status = _rows(cs, nb, F)
    assert len(names) == 30 and np.diff(fp).tolist() == [1, 1, 0, 27, 1]
    assert status[names.index("zero")] == 3 and status[names.index("iteration limit")] == 2
    assert (np.abs(shape[[n == "elliptical" for n in names], 3]) > 0.1).all()
    ref = bo.blend(stamps, shape, status, places, T, D, fp)
    assert ref["npix"][names.index("zero")] == -1 and ref["npix"][names.index("iteration limit")] == cs * cs
    assert [ref["npix"][i] for i, n in enumerate(names) if n == "outside"] == [0, 0]
    assert 0 < ref["npix"][names.index("alone corner")] < cs * cs and 0 < ref["npix"][names.index("alone edge")] < cs * cs
    assert 0 < ref["npix"][names.index("corner")] < cs * cs

    got = _ctx().scene_blend(stamps, shape, status, places, T, D, field_ptr=fp)
    assert got["blend"].shape == (30, 4) and got["npix"].dtype == np.int32
    scale = np.concatenate([ref["blend"][:, :1], ref["abs"]], axis=1)            # W is its own absolute sum
    err = np.abs(got["blend"] - ref["blend"])
    for i, name in enumerate(names):
        rel = err[i] / np.where(scale[i] > 0, scale[i], 1.0)
        print(f"{cs}/{nb} galaxy {i:2d} {name:15s}: npix {got['npix'][i]:5d}, W A Bm Bd off by {np.array2string(rel, precision=1)} "
              f"of sum g |x|, blendedness {1 - got['blend'][i, 1] / got['blend'][i, 2] if got['blend'][i, 2] > 0 else np.nan:.6f}")
    assert np.array_equal(got["npix"], ref["npix"])
    assert np.array_equal(np.isnan(got["blend"]), np.isnan(ref["blend"]))
    assert np.isnan(ref["blend"]).sum() == 4                                      # the zero stamp's row, nothing else
    fin = ~np.isnan(ref["blend"])
    assert (err[fin] <= 1e-12 * scale[fin]).all()
    # alone in its field, clipped or not: T holds the widened stamp values and the two sums have the same bits
    alone = [i for i, n in enumerate(names) if n.startswith("alone")]
    assert len(alone) == 3
    for i in alone:
        assert got["blend"][i, 1] == got["blend"][i, 2] and got["blend"][i, 1] > 0, names[i]
    crowd = [i for i, n in enumerate(names) if n in ("pair a", "pair b", "triple")]
    assert (got["blend"][crowd, 2] > got["blend"][crowd, 1]).all()
    # without data fields: Bd is NaN, the rest has the same bits
    bare = _ctx().scene_blend(stamps, shape, status, places, T, field_ptr=fp)
    assert np.isnan(bare["blend"][:, 3]).all() and np.array_equal(bare["blend"][:, :3], got["blend"][:, :3], equal_nan=True)
    assert np.array_equal(bare["npix"], got["npix"])
    # a row does not depend on where its galaxy or its field sits in the batch: the fields in reverse order
    order = np.concatenate([np.arange(fp[m], fp[m + 1]) for m in range(4, -1, -1)])
    fp_r = np.concatenate([[0], np.cumsum(np.diff(fp)[::-1])])
    moved = _ctx().scene_blend(stamps[order], shape[order], status[order], places[order], T[::-1], D[::-1], field_ptr=fp_r)
    assert np.array_equal(moved["blend"], got["blend"][order], equal_nan=True) and np.array_equal(moved["npix"], got["npix"][order])
    one = _ctx().scene_blend(stamps[5:6], shape[5:6], status[5:6], places[5:6], T[3:4], D[3:4])      # one galaxy of the crowd
    assert np.array_equal(one["blend"], got["blend"][5:6]) and one["npix"][0] == got["npix"][5]


# ---- part 2: the pipeline -----------------------------------------------------------------------------------------------
CS, NB, F2 = 31, 6, 131
ARCH = dict(input_shape=(CS, CS, NB), latent_dim=32, filters=[32, 64, 128], kernels=[3, 3, 3])
COUNTS = [30, 0, 150, 7, 40]      # one empty field, one with more stamps than max_batch = 64: chunks cross field boundaries
CAT = ("flux", "flux_err", "shape", "iters", "status")
BLEND = ("blend", "npix")


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _blob_fields(M, seed, nblob=14):
    rng = np.random.default_rng(seed)
    out = rng.normal(0, 0.05, size=(M, F2, F2, NB))
    yy, xx = np.mgrid[:F2, :F2]
    for m in range(M):
        for _ in range(nblob):
            r, c = rng.uniform(15, F2 - 15, size=2)
            sig, a = rng.uniform(1.5, 3.0), rng.uniform(2.0, 9.0)
            out[m] += (a * np.exp(-0.5 * ((yy - r) ** 2 + (xx - c) ** 2) / sig ** 2))[:, :, None] * rng.uniform(0.5, 1.0, size=NB)
    return out


def _windows(counts, seed):
    rng = np.random.default_rng(seed)
    n = int(np.sum(counts))
    starts = rng.integers(0, F2 - CS + 1, size=(n, 2)).astype(np.int32)
    places = starts.copy()
    k = rng.random(n) < 0.3                                          # some hang over an edge, a few lie wholly outside
    places[k] = rng.integers(-CS - 2, F2 + 2, size=(int(k.sum()), 2))
    return starts, places, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _net(dtype):
    from debvader_amd.model import model

    net, _, _, _ = model.create_model_vae(**ARCH, max_batch=64, seed=3, dtype=dtype)
    return net


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_stamp_level_call(dtype, monkeypatch):
    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(5, seed=11)
    starts, places, fp = _windows(COUNTS, seed=5)
    seed = 77

    def reference(fields, starts, places, fp):
        stamps = eng.infer_fields(fields, starts, fp, seed=seed)["loc"]
        rows = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
        comp = eng.infer_fields_composite(fields, starts, places, fp, seed=seed)
        assert np.array_equal(rows["mean_fields"], comp["mean_fields"])
        want = ctx.scene_blend(stamps, rows["shape"], rows["status"], places, comp["mean_fields"], fields, field_ptr=fp)
        return rows, want

    rows, want = reference(fields, starts, places, fp)
    ok = want["npix"] >= 0
    print(f"[{dtype}] {int(ok.sum())} eligible of {len(ok)} galaxies, {int((want['npix'] == 0).sum())} wholly outside, "
          f"{int(((want['npix'] > 0) & (want['npix'] < CS * CS)).sum())} clipped; blendedness "
          f"{np.nanmin(1 - want['blend'][ok, 1] / want['blend'][ok, 2]):.3f} .. "
          f"{np.nanmax(1 - want['blend'][ok, 1] / want['blend'][ok, 2]):.3f}")
    assert ok.sum() >= 100 and ((want["npix"] > 0) & (want["npix"] < CS * CS)).any()

    got = eng.infer_fields_measure_blend(fields, starts, fp, places, seed=seed)
    assert sorted(got) == sorted(tuple(rows) + BLEND)
    for k in BLEND:
        assert _eq(got[k], want[k]), k
    for k in rows:                                                   # every shared output has infer_fields_measure's bits
        assert _eq(got[k], rows[k]), k
    # catalogue-only: the mean field is composited on the device and stays there
    only = eng.infer_fields_measure_blend(fields, starts, fp, places, seed=seed, return_fields=False)
    assert sorted(only) == sorted(CAT + ("mse_center",) + BLEND)
    for k in only:
        assert _eq(only[k], got[k]), k
    # grouped: three resident fields at a time, so chunks 0-1 run with fields 0 .. 2 and chunks 2-3 with fields 2 .. 4 -
    # field 2 is carried, its parent sums run in the second group (a field is 824 KB: 4 per field with the result fields,
    # 2 catalogue-only).
    # That exactly three fields are resident is observed, not assumed: one MiB less holds only two, and the call is then
    # refused because chunk 0 (stamps 0 .. 63) spans fields 0 .. 2.  So per_field > limit / 3 at the lower limit, which
    # leaves fewer than four at the higher one; with three resident and stamps in fields 0, 2, 3, 4 no group holds them
    # all, and a boundary - on a chunk of 64 - before stamp 180 (field 3) falls at stamp 64 or 128, inside field 2.
    from debvader_amd._lib import DvError

    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "9")
    with pytest.raises(DvError, match="come from 3 fields, device memory holds 2"):
        eng.infer_fields_measure_blend(fields, starts, fp, places, seed=seed)
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "10")
    grouped = eng.infer_fields_measure_blend(fields, starts, fp, places, seed=seed)
    for k in got:
        assert _eq(grouped[k], got[k]), k
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "4")
    with pytest.raises(DvError, match="come from 3 fields, device memory holds 2"):
        eng.infer_fields_measure_blend(fields, starts, fp, places, seed=seed, return_fields=False)
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "5")
    g2 = eng.infer_fields_measure_blend(fields, starts, fp, places, seed=seed, return_fields=False)
    for k in only:
        assert _eq(g2[k], only[k]), k
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    # the fields permuted: the noise rows move with the stamp numbers, so the reference is taken again; a galaxy alone in
    # the call's arithmetic either way
    perm = [3, 2, 0, 4, 1]
    order = np.concatenate([np.arange(fp[m], fp[m + 1]) for m in perm])
    fp_p = np.concatenate([[0], np.cumsum(np.array(COUNTS)[perm])]).astype(np.int64)
    rows_p, want_p = reference(fields[perm], starts[order], places[order], fp_p)
    for rf in (True, False):
        got_p = eng.infer_fields_measure_blend(fields[perm], starts[order], fp_p, places[order], seed=seed, return_fields=rf)
        for k in BLEND:
            assert _eq(got_p[k], want_p[k]), (rf, k)
        for k in got_p:
            if k not in BLEND:
                assert _eq(got_p[k], rows_p[k]), (rf, k)
    # one field alone (M = 1) under its singular names, and the tiny call of 7 stamps
    for m in (2, 3):
        s1, p1 = starts[fp[m]:fp[m + 1]], places[fp[m]:fp[m + 1]]
        fp1 = np.array([0, len(s1)], np.int64)
        rows_1, want_1 = reference(fields[m:m + 1], s1, p1, fp1)
        one = eng.infer_cutouts_measure_blend(fields[m], s1, p1, seed=seed)
        assert "mean_field" in one and np.array_equal(one["mean_field"], rows_1["mean_fields"][0])
        for k in BLEND:
            assert _eq(one[k], want_1[k]), (m, k)
        for k in CAT + ("mse_center",):
            assert _eq(one[k], rows_1[k]), (m, k)
        only_1 = eng.infer_cutouts_measure_blend(fields[m], s1, p1, seed=seed, return_fields=False)
        assert all(_eq(only_1[k], one[k]) for k in only_1) and sorted(only_1) == sorted(CAT + ("mse_center",) + BLEND)


def test_deblend_field_batch_blendedness_on_the_device():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure.measurement import blend_dtype, measure_blendedness

    fields = _blob_fields(3, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-45, 46, size=(n, 2)).astype(np.float64) for n in (20, 0, 75)]

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds
        return DeblendFieldBatch(net, fields, CS, NB)

    a, b, c, d = batch(), batch(), batch(), batch()
    res = a.deblend_fields(dists, on_device=True, measure=True, blendedness=True)
    plain = b.deblend_fields(dists, on_device=True, measure=True)
    host = c.deblend_fields(dists, measure=True)                  # the default path: stamps and catalogue on the host
    model = c.get_predicted_fields()["predicted_mean_fields"]
    assert np.array_equal(model, a.get_predicted_fields()["predicted_mean_fields"])
    names = tuple(n for n, _ in blend_dtype())
    for m, (r, p, h) in enumerate(zip(res, plain, host)):
        assert r.dtype == np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + blend_dtype())
        for k in p.dtype.names:                                   # the columns of the call without it, value for value
            if k == "shifts":
                assert all(np.array_equal(x, y) for x, y in zip(r[k], p[k]))
            else:
                assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].kind == "f"), k
        if not len(r):
            continue
        stamps = np.stack([np.asarray(x) for x in h["output_images_mean"]])
        places = int((F2 - CS) / 2) + dists[m].astype(np.int64)
        want = measure_blendedness(stamps, h, places, model[m], fields[m], ctx=c._ctx)
        for k in names:
            assert np.array_equal(r[k], want[k], equal_nan=True), (m, k)
        ok = r["blend_npix"] > 0
        assert ok.sum() >= len(r) // 2 and (r["blendedness"][ok] > -1e-12).all() and (r["blendedness"][ok] < 1).all()
    cat = d.deblend_fields(dists, on_device=True, measure=True, blendedness=True, return_fields=False)
    for r, q in zip(res, cat):
        for k in r.dtype.names:
            if k != "shifts":
                assert np.array_equal(r[k], q[k], equal_nan=r.dtype[k].kind == "f"), k


def test_refusals_come_before_any_gpu_work_and_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import Engine, _dp, _fp, _ip

    DvError, lib = _lib.DvError, _lib.lib
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(1, seed=11)
    starts, places, fp = _windows([5], seed=5)
    good = eng.infer_fields_measure_blend(fields, starts, fp, places, seed=3)
    n = 5
    flux, ferr, shape = np.zeros((n, NB)), np.zeros((n, NB)), np.zeros((n, 5))
    iters, status, blend, npix = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 4)), np.zeros(n, np.int32)
    f2, N, args = Engine._field_args(fields, starts, fp, places)
    cat = (_dp(flux), _dp(ferr), _dp(shape), _ip(iters), _ip(status))

    def pipeline(par, args=args, cat=cat, out=(_dp(blend), _ip(npix))):
        _lib.check(lib.dv_infer_fields_measure_blend(eng._h, *args, 9, C.byref(par), None, None, None, None, *cat, *out))

    par = _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
    for bad in (_lib.DvMeasureParams(NB, 3.0, 1e-10, 200), _lib.DvMeasureParams(2, 0.0, 1e-10, 200)):
        with pytest.raises(DvError, match="band|sigma0"):                       # what dv_infer_fields_measure refuses
            pipeline(bad)
    with pytest.raises(DvError, match="must all be given"):
        pipeline(par, cat=(None,) + cat[1:])
    with pytest.raises(DvError, match="places, blend and npix"):
        pipeline(par, args=args[:5] + [None] + args[6:])
    with pytest.raises(DvError, match="places, blend and npix"):
        pipeline(par, out=(None, _ip(npix)))
    with pytest.raises(DvError, match="places, blend and npix"):
        pipeline(par, out=(_dp(blend), None))
    # the stamp-level call
    st = np.zeros((2, CS, CS, 3), np.float32)
    sh, ss, pl, T = np.zeros((2, 5)), np.zeros(2, np.int32), np.zeros((2, 2), np.int32), np.zeros((1, 40, 40, 3))
    bl, npx, fp2 = np.zeros((2, 4)), np.zeros(2, np.int32), np.array([0, 2], np.int64)

    def stamps(band=2, cs=CS, nb=3, ptr=fp2, out=(_dp(bl), _ip(npx)), sh_=sh):
        _lib.check(lib.dv_scene_blend(ctx._h, _fp(st), _dp(sh_), _ip(ss), _ip(pl), ptr.ctypes.data_as(C.POINTER(C.c_int64)), 2,
                                      cs, nb, band, _dp(T), None, 1, 40, *out))

    for kw, msg in [(dict(band=3), "band"), (dict(cs=4097), "4096 pixels"), (dict(cs=0), "4096 pixels"), (dict(nb=0), "bands"),
                    (dict(out=(None, _ip(npx))), "must all"), (dict(sh_=None), "must all"),
                    (dict(ptr=np.array([0, 1], np.int64)), "field_ptr")]:
        with pytest.raises(DvError, match=msg):
            stamps(**kw)
    # a table that overshoots before it decreases passes both end checks: it is refused before anything is indexed by it
    T2 = np.zeros((2, 40, 40, 3))
    with pytest.raises(DvError, match="field_ptr decreases at field 1"):
        _lib.check(lib.dv_scene_blend(ctx._h, _fp(st), _dp(sh), _ip(ss), _ip(pl),
                                      np.array([0, 1 << 40, 2], np.int64).ctypes.data_as(C.POINTER(C.c_int64)), 2, CS, 3, 2,
                                      _dp(T2), None, 2, 40, _dp(bl), _ip(npx)))
    # the engine completes a correct call afterwards
    pipeline(par)
    again = eng.infer_fields_measure_blend(fields, starts, fp, places, seed=3)
    for k in good:
        assert _eq(again[k], good[k]), k
    assert _eq(blend, eng.infer_fields_measure_blend(fields, starts, fp, places, seed=9, return_fields=False)["blend"])
