"""The simultaneous flux fit on the GPU (dv_scene_fit_flux, dv_scene_fit_flux_gram, dv_infer_fields_measure_fit,
DeblendFieldBatch(fit_flux=True)).  Part 1: the host-array call against the numpy restatement of
tests/fit_flux_oracle.py.  The restatement factorises in another order of additions than the kernel, so the comparison is one
of bounds, and it is only valid where the bounds were derived: the test first asserts, on the CPU, that the diagonally scaled
Gram matrix of every field and band has a condition number below 100.  Then: the zero pattern of G, the statuses and the NaN
pattern are equal bit for bit; fit_gram and fit_proj lie within 1e-12 of the sums of their absolute terms (at most cs^2 = 3481
terms times 2^-53 is 4e-13 for any summation order); the backward error of the solve is below 1e-10 (the Cholesky bound is of
order n^2 2^-53 = 2e-13 at n = 40); fit_scale lies within 1e-10 max|a| of numpy.linalg.solve and fit_var within 1e-9 relative
of numpy.linalg.inv on the restatement's G (expected: cond n 2^-53 = 4e-13).  The worst ratio met is printed for each bound.
Part 2: the pipeline stage against the host call, bit for bit, on both engines."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import fit_flux_oracle as fo
from tests.test_gpu_aperture import CAT, COUNTS, CS, NB, _blob_fields, _net, _windows
from tests.test_gpu_blend import _scene as _blend_scene

pytestmark = pytest.mark.gpu

KEYS = ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status")
NBIG = 40


def _ctx():
    from debvader_amd import engine as E

    return E.default_context()


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


@functools.lru_cache(maxsize=None)
def _scene(cs, nb, F):
    """Six fields, 71 galaxies: (names, stamps float32, places, field_ptr, D); never written to.  The 30 galaxies of
    tests/test_gpu_blend.py - one alone inside its field, one alone over a corner, a field without stamps, the crowd (lone
    galaxies, pairs, a triple, a stamp over a corner, two stamps wholly outside, an all-zero stamp, elliptical blobs), and
    last one alone at an edge - with an exact duplicate of the first "pair b" galaxy behind the crowd, and before the last
    field a crowded one: 40 random elliptical blobs, some over the edges.  D is the composite of the stamps at random true
    amplitudes plus noise."""
    names, stamps, places, fp, _, _ = _blend_scene(cs, nb, F)
    names, stamps, places, fp = list(names), np.array(stamps), np.array(places), np.array(fp)
    at, src = int(fp[4]), names.index("pair b")
    names = names[:at] + ["duplicate"] + names[at:]
    stamps = np.concatenate([stamps[:at], stamps[src:src + 1], stamps[at:]])
    places = np.concatenate([places[:at], places[src:src + 1], places[at:]])
    fp[4:] += 1
    rng = np.random.default_rng(4000 + cs)
    s = cs / 31.0
    big = np.zeros((NBIG, cs, cs, nb), np.float32)
    for i in range(NBIG):
        a, b = rng.uniform(1.5, 5.0, size=2) * s * s
        M = (a, rng.choice([-1.0, 1.0]) * rng.uniform(0.1, 0.6) * np.sqrt(a * b), b)
        p = fo.elliptical_gaussian(cs, M, rng.uniform(-2.0, 2.0, size=2) * s, rng.uniform(0.5, 3.0))
        big[i] = (p[:, :, None] * rng.uniform(0.3, 2.0, size=nb) + rng.uniform(0.0, 0.01, size=(cs, cs, nb))).astype(np.float32)
    # on a jittered 7 x 6 grid that overhangs the field: neighbours overlap, nobody coincides
    cells = rng.permutation(42)[:NBIG]
    step = (F - cs // 2) / 7.0
    big_places = np.stack([(cells // 6) * step - cs // 4 + rng.uniform(-0.2, 0.2, NBIG) * step,
                           (cells % 6) * (step * 7 / 6) - cs // 4 + rng.uniform(-0.2, 0.2, NBIG) * step], axis=1).astype(np.int32)
    at = int(fp[4])                                                # before the last field
    names = names[:at] + ["crowded"] * NBIG + names[at:]
    stamps = np.concatenate([stamps[:at], big, stamps[at:]])
    places = np.concatenate([places[:at], big_places, places[at:]]).astype(np.int32)
    fp = np.concatenate([fp[:5], [fp[4] + NBIG], fp[5:] + NBIG]).astype(np.int64)
    amps = rng.uniform(0.7, 1.3, size=len(names))
    D = np.zeros((6, F, F, nb))
    for m in range(6):
        for i in range(int(fp[m]), int(fp[m + 1])):
            ra, rz, ca, cz = fo.clip(places[i], cs, F)
            if rz > ra and cz > ca:
                pr, pc = places[i]
                D[m, ra:rz, ca:cz] += amps[i] * stamps[i, ra - pr:rz - pr, ca - pc:cz - pc].astype(np.float64)
    D += rng.normal(0.0, 0.05, size=D.shape)
    for a in (stamps, places, fp, D):
        a.flags.writeable = False
    return names, stamps, places, fp, D


@functools.lru_cache(maxsize=None)
def _ref(cs, nb, F):
    """the restatement of the scene, computed once"""
    _, stamps, places, fp, D = _scene(cs, nb, F)
    out, fields = fo.fit_flux(stamps, places, fp, D)
    for a in out.values():
        a.flags.writeable = False
    return out, fields


@functools.lru_cache(maxsize=None)
def _gpu(cs, nb, F):
    _, stamps, places, fp, D = _scene(cs, nb, F)
    out = _ctx().scene_fit_flux(stamps, places, D, field_ptr=fp)
    for a in out.values():
        a.flags.writeable = False
    return out


SHAPES = [(31, 3, 64), (59, 6, 97)]


@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_scene_fit_flux_against_the_restatement(cs, nb, F):
    names, stamps, places, fp, D = _scene(cs, nb, F)
    assert len(names) == 71 and np.diff(fp).tolist() == [1, 1, 0, 28, NBIG, 1]
    ref, fields = _ref(cs, nb, F)
    # the oracle is in its safe regime: every kept system is well conditioned once scaled to a unit diagonal
    conds = [fo.scaled_condition(s["full"], s["kept"]) for f in fields for s in f["bands"]]
    print(f"{cs}/{nb}: scaled condition numbers up to {max(conds):.1f}")
    assert max(conds) < 100.0
    got = _gpu(cs, nb, F)
    assert sorted(got) == sorted(KEYS) and all(got[k].shape == (71, nb) for k in KEYS) and got["fit_status"].dtype == np.int32
    # the statuses and the NaN pattern, bit for bit
    assert np.array_equal(got["fit_status"], ref["fit_status"])
    for k in ("fit_scale", "fit_var", "fit_gram", "fit_proj"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
    st = dict(zip(names, got["fit_status"]))
    assert (st["zero"] == 4).all() and (st["duplicate"] == 5).all() and (st["alone corner"] == 0).all()
    out_rows = [i for i, n in enumerate(names) if n == "outside"]
    assert (got["fit_status"][out_rows] == 4).all() and (got["fit_gram"][out_rows] == 0.0).all() and (got["fit_proj"][out_rows] == 0.0).all()
    assert np.bincount(got["fit_status"].ravel(), minlength=6).tolist() == [67 * nb, 0, 0, 0, 3 * nb, nb]
    dup = names.index("duplicate")
    assert (got["fit_scale"][dup] == 1.0).all() and np.isnan(got["fit_var"][dup]).all()
    assert np.array_equal(got["fit_gram"][dup], got["fit_gram"][names.index("pair b")])
    # step 1: the sums within 1e-12 of the sums of their absolute terms
    worst = {}
    for k, a in (("fit_gram", "gram_abs"), ("fit_proj", "proj_abs")):
        err = np.abs(got[k] - ref[k])
        assert (err <= 1e-12 * ref[a]).all(), k
        worst[k] = float((err / np.where(ref[a] > 0, ref[a], 1.0)).max() / 1e-12)
    # the whole Gram matrix of every field: the zero pattern bit for bit, the entries by the same bound
    worst["G"] = 0.0
    for m, f in enumerate(fields):
        lo, hi = int(fp[m]), int(fp[m + 1])
        g = _ctx().scene_fit_flux_gram(stamps[lo:hi], places[lo:hi], D[m])
        assert g["gram"].shape == (nb, hi - lo, hi - lo) and np.array_equal(g["gram"] == 0.0, f["G"] == 0.0), m
        assert (np.abs(g["gram"] - f["G"]) <= 1e-12 * f["Gabs"]).all(), m
        if hi > lo:
            worst["G"] = max(worst["G"], float((np.abs(g["gram"] - f["G"]) / np.where(f["Gabs"] > 0, f["Gabs"], 1.0)).max() / 1e-12))
        # the fit works on these bits
        assert np.array_equal(np.diagonal(g["gram"], axis1=1, axis2=2).T, got["fit_gram"][lo:hi])
        assert np.array_equal(g["proj"], got["fit_proj"][lo:hi])
    assert (fields[3]["G"][0] == 0.0).sum() > 28 * 27 // 2           # (the crowd has pairs that do not overlap)
    # steps 2 - 5 per field and band
    worst.update(backward=0.0, scale=0.0, var=0.0)
    for m, f in enumerate(fields):
        lo = int(fp[m])
        for b, s in enumerate(f["bands"]):
            kept = s["kept"]
            if not len(kept):
                continue
            A, hp = s["full"][np.ix_(kept, kept)], s["hp"]
            a, v = got["fit_scale"][lo + kept, b], got["fit_var"][lo + kept, b]
            back = np.abs(A @ a - hp).max()
            bound = 1e-10 * (np.abs(A).sum(axis=1).max() * np.abs(a).max() + np.abs(hp).max())
            assert back <= bound, (m, b, back, bound)
            worst["backward"] = max(worst["backward"], back / bound)
            want = np.linalg.solve(A, hp)
            assert (np.abs(a - want) <= 1e-10 * np.abs(want).max()).all(), (m, b)
            worst["scale"] = max(worst["scale"], np.abs(a - want).max() / (1e-10 * np.abs(want).max()))
            wv = np.diagonal(np.linalg.inv(A))
            assert (np.abs(v - wv) <= 1e-9 * wv).all(), (m, b)
            worst["var"] = max(worst["var"], (np.abs(v - wv) / wv).max() / 1e-9)
            assert (v >= 1.0 / np.diagonal(A) * (1.0 - 1e-12)).all()      # a neighbour never helps
    print(f"{cs}/{nb}: worst fraction of each bound - " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    # the fit finds the amplitudes the data were made with, within the noise
    big = slice(int(fp[4]), int(fp[5]))
    err = got["fit_scale"][big] - np.clip(got["fit_scale"][big], 0.7, 1.3)
    assert (np.abs(err) <= 6.0 * 0.05 * np.sqrt(got["fit_var"][big])).all()


@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_rows_keep_their_bits(cs, nb, F):
    from debvader_amd._lib import DvError

    names, stamps, places, fp, D = _scene(cs, nb, F)
    ctx = _ctx()
    got = _gpu(cs, nb, F)
    again = ctx.scene_fit_flux(stamps, places, D, field_ptr=fp)
    for k in KEYS:
        assert _eq(again[k], got[k]), k
    # the fields in reverse order
    order = np.concatenate([np.arange(fp[m], fp[m + 1]) for m in range(5, -1, -1)])
    fp_r = np.concatenate([[0], np.cumsum(np.diff(fp)[::-1])])
    moved = ctx.scene_fit_flux(stamps[order], places[order], D[::-1], field_ptr=fp_r)
    for k in KEYS:
        assert _eq(moved[k], got[k][order]), k
    # one field alone in the call
    for m in (0, 3, 4):
        lo, hi = int(fp[m]), int(fp[m + 1])
        one = ctx.scene_fit_flux(stamps[lo:hi], places[lo:hi], D[m:m + 1])
        for k in KEYS:
            assert _eq(one[k], got[k][lo:hi]), (m, k)
    # a scratch that holds the crowded field and no more: fields 0 .. 3, field 4 and field 5 go through it one after another
    tight = nb * NBIG * NBIG * 8
    assert nb * 28 * 28 * 8 + 2 * nb * 8 < tight
    split = ctx.scene_fit_flux(stamps, places, D, field_ptr=fp, scratch_bytes=tight)
    for k in KEYS:
        assert _eq(split[k], got[k]), k
    # one byte less and the crowded field does not fit: refused by name, and the engine gives the bits it gave before
    with pytest.raises(DvError, match=rf"field 4 has {NBIG} galaxies.*{tight} bytes of scratch.*scratch_bytes is {tight - 1}"):
        ctx.scene_fit_flux(stamps, places, D, field_ptr=fp, scratch_bytes=tight - 1)
    if cs == 31:                                                   # (one shape: the refusal does not depend on it)
        many = 1025                                                # a chain of stamps that overlap their neighbours by one pixel
        chain = np.stack([np.zeros(many), (np.arange(many) % 3) * (cs - 1)], axis=1).astype(np.int32)
        with pytest.raises(DvError, match="field 1 has 1025 galaxies, the dense fit takes at most 1024"):
            ctx.scene_fit_flux(np.concatenate([stamps[:1], np.ones((many, cs, cs, nb), np.float32)]),
                               np.concatenate([places[:1], chain]), np.ones((2, F, F, nb)), field_ptr=[0, 1, 1 + many])
    again = ctx.scene_fit_flux(stamps, places, D, field_ptr=fp)
    for k in KEYS:
        assert _eq(again[k], got[k]), k
    # another min_pivot reaches the kernel: a generous one drops members of the crowd
    loose = ctx.scene_fit_flux(stamps, places, D, field_ptr=fp, min_pivot=0.9)
    assert (loose["fit_status"] == 5).sum() > (got["fit_status"] == 5).sum() and _eq(loose["fit_gram"], got["fit_gram"])


def test_a_field_of_more_galaxies_than_threads():
    """300 small stamps on a 3-pixel grid, one band: every loop of the solve kernel that strides over 64 lanes or 256 threads
    takes more than one turn, and with one band no two floats of a pixel share an 8-byte load.  The 4- and 8-neighbour
    overlaps give a scaled condition number near 6; numpy solves the GPU's own Gram matrix."""
    cs, F, n = 9, 64, 300
    rng = np.random.default_rng(9)
    cells = np.arange(n)
    places = np.stack([(cells // 18) * 3, (cells % 18) * 3], axis=1).astype(np.int32)
    places[:4] = [[-4, -4], [F - 5, 2], [3, F - 4], [F - 6, F - 6]]                 # (some over the edges)
    stamps = np.stack([fo.elliptical_gaussian(cs, (1.4, rng.uniform(-0.3, 0.3), 1.4), rng.uniform(-0.5, 0.5, 2), rng.uniform(0.5, 2.0))
                       for _ in range(n)])[..., None].astype(np.float32)
    D = rng.normal(0.0, 0.05, size=(F, F, 1))
    for i in range(n):
        ra, rz, ca, cz = fo.clip(places[i], cs, F)
        D[ra:rz, ca:cz] += stamps[i, ra - places[i, 0]:rz - places[i, 0], ca - places[i, 1]:cz - places[i, 1]].astype(np.float64)
    ctx = _ctx()
    got = ctx.scene_fit_flux(stamps, places, D[None])
    g = ctx.scene_fit_flux_gram(stamps, places, D)
    A = np.tril(g["gram"][0]) + np.tril(g["gram"][0], -1).T
    d = 1.0 / np.sqrt(np.diagonal(A))
    cond = np.linalg.cond(A * d[:, None] * d[None, :])
    assert cond < 100.0 and (got["fit_status"] == 0).all()
    assert np.array_equal(np.diagonal(A), got["fit_gram"][:, 0]) and np.array_equal(g["proj"], got["fit_proj"])
    a, v, h = got["fit_scale"][:, 0], got["fit_var"][:, 0], g["proj"][:, 0]
    want, wv = np.linalg.solve(A, h), np.diagonal(np.linalg.inv(A))
    back, bound = np.abs(A @ a - h).max(), 1e-10 * (np.abs(A).sum(axis=1).max() * np.abs(a).max() + np.abs(h).max())
    print(f"n = {n}: condition {cond:.1f}; fraction of each bound - backward {back / bound:.1e}, scale "
          f"{np.abs(a - want).max() / (1e-10 * np.abs(want).max()):.1e}, var {(np.abs(v - wv) / wv).max() / 1e-9:.1e}")
    assert back <= bound
    assert (np.abs(a - want) <= 1e-10 * np.abs(want).max()).all() and (np.abs(v - wv) <= 1e-9 * wv).all()
    assert np.abs(a - 1.0).max() < 0.5
    # the restatement agrees on step 1 for a few rows of it
    G, Ga, hh, ha = fo.gram_field(stamps[:40], places[:40], D)
    assert np.array_equal(g["gram"][0, :40, :40] == 0.0, G[0] == 0.0) and (np.abs(g["gram"][0, :40, :40] - G[0]) <= 1e-12 * Ga[0]).all()


# ---- part 2: the pipeline -----------------------------------------------------------------------------------------------------
F2 = 131


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_host_call(dtype, monkeypatch):
    from debvader_amd._lib import DvError

    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(5, F2, seed=11)
    starts, places, fp = _windows(F2, COUNTS, seed=5)
    seed = 77
    stamps = eng.infer_fields_keep(fields, starts, fp, seed=seed)["loc"]
    want = ctx.scene_fit_flux(stamps, places, fields, field_ptr=fp)
    rows = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    print(f"[{dtype}] fit_status of the {len(starts)} network stamps x {NB} bands: "
          f"{np.bincount(want['fit_status'].ravel(), minlength=6).tolist()}")
    assert (want["fit_status"] == 0).any()

    got = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=seed)
    assert sorted(got) == sorted(tuple(rows) + KEYS)
    for k in KEYS:
        assert _eq(got[k], want[k]), k
    for k in rows:                                                # every shared output has infer_fields_measure's bits
        assert _eq(got[k], rows[k]), k
    # catalogue-only: no field is composited
    only = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=seed, return_fields=False)
    assert sorted(only) == sorted(CAT + ("mse_center",) + KEYS)
    for k in only:
        assert _eq(only[k], got[k]), k
    plain = eng.infer_fields_measure(fields, starts, fp, seed=seed, return_fields=False)
    for k in plain:
        assert _eq(only[k], plain[k]), k
    # grouped: a field is 824 KB, four per resident field with the result fields - 10 MiB hold three, so field 2 (stamps 30 ..
    # 179, chunks of 64) is carried from the first group into the second and its fit runs there.  The catalogue-only form keeps
    # the source field alone: 5 MiB hold all five fields, 3 MiB three of them - field 2 is carried again - and 2 MiB too few
    # for chunk 0, which spans three
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "10")
    grouped = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=seed)
    for k in got:
        assert _eq(grouped[k], got[k]), k
    for mb in ("5", "3"):
        monkeypatch.setenv("DV_FIELDS_GROUP_MB", mb)
        g2 = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=seed, return_fields=False)
        for k in only:
            assert _eq(g2[k], only[k]), (mb, k)
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "2")
    with pytest.raises(DvError, match="come from 3 fields, device memory holds 2"):
        eng.infer_fields_measure_fit(fields, starts, fp, places, seed=seed, return_fields=False)
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    # a scratch that takes the 150-stamp field alone: three sub-ranges at the seam, the same bits; other parameters reach the
    # kernel; M = 1 is the single-field view
    tight = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=seed, return_fields=False, scratch_bytes=NB * 150 * 150 * 8)
    for k in only:
        assert _eq(tight[k], only[k]), k
    loose = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=seed, return_fields=False, min_pivot=0.5, band=0, max_iter=9)
    w2 = ctx.scene_fit_flux(stamps, places, fields, field_ptr=fp, min_pivot=0.5)
    assert all(_eq(loose[k], w2[k]) for k in KEYS) and not _eq(loose["shape"], only["shape"])
    m = 3
    s1, p1 = starts[fp[m]:fp[m + 1]], places[fp[m]:fp[m + 1]]
    one = eng.infer_cutouts_measure_fit(fields[m], s1, p1, seed=seed)
    st1 = eng.infer_fields_keep(fields[m:m + 1], s1, [0, len(s1)], seed=seed)["loc"]
    w1 = ctx.scene_fit_flux(st1, p1, fields[m:m + 1])
    assert "mean_field" in one and all(_eq(one[k], w1[k]) for k in KEYS)


def test_deblend_field_batch_takes_the_flux_fit():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    fields = _blob_fields(3, F2, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-45, 46, size=(n, 2)).astype(np.float64) for n in (20, 0, 45)]
    sky = np.linspace(0.03, 0.06, 3 * NB).reshape(3, NB)

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds
        return DeblendFieldBatch(net, fields, CS, NB)

    a, b, c, d = batch(), batch(), batch(), batch()
    res = a.deblend_fields(dists, on_device=True, measure=True, fit_flux=True, sky_sigma=sky)
    plain = b.deblend_fields(dists, on_device=True, measure=True)
    host = c.deblend_fields(dists, measure=True)                  # the default path: stamps and catalogue on the host
    names = tuple(n[0] for n in ms.fit_flux_dtype(NB))
    want_cols = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + DeblendFieldBatch.fit_flux_columns(NB))
    for m, (r, p, h) in enumerate(zip(res, plain, host)):
        assert r.dtype == want_cols and len(r) == len(p)
        for k in p.dtype.names:                                   # the columns of the call without it, value for value
            if k != "shifts":
                assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].base.kind == "f"), k
        if not len(r):
            continue
        mean = np.stack([np.asarray(x) for x in h["output_images_mean"]])
        places = int((F2 - CS) / 2) + dists[m].astype(np.int64)
        want = ms.fit_fluxes(mean, places, fields[m], catalogue=h, sky_sigma=sky[m], ctx=c._ctx)
        for k in names:
            assert np.array_equal(r[k], want[k], equal_nan=True), (m, k)
        ok = r["fit_status"] == 0
        assert ok.any() and np.isfinite(r["flux_fit"][ok]).all() and (r["fit_scale_err"][ok] > 0).all()
        assert ((r["fit_independence"][ok] > 0) & (r["fit_independence"][ok] <= 1.0 + 1e-12)).all()
    cat = d.deblend_fields(dists, on_device=True, measure=True, fit_flux=True, sky_sigma=sky, return_fields=False)
    for r, q in zip(res, cat):
        for k in r.dtype.names:
            if k != "shifts":
                assert np.array_equal(r[k], q[k], equal_nan=r.dtype[k].base.kind == "f"), k


def test_refusals_come_before_any_gpu_work_and_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import Engine, _dp, _fp, _ip, fit_flux_params

    DvError, lib = _lib.DvError, _lib.lib
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(1, F2, seed=11)
    starts, places, fp = _windows(F2, [5], seed=5, hang=False)
    good = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=3)

    n, nb = 5, NB
    ptr = lambda a: None if a is None else (_dp(a) if a.dtype == np.float64 else _fp(a) if a.dtype == np.float32 else _ip(a))   # noqa: E731
    cat = [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    five = lambda n, nb: [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb), np.int32)]   # noqa: E731
    ff = five(n, nb)
    f2, N, args = Engine._field_args(fields, starts, fp, places)
    mean_f, std_f, res_f = np.empty(f2.shape), np.empty(f2.shape), np.empty(f2.shape)

    def pipeline(par=None, fpar=None, out=None, fields_out=(None, None, None), no_params=False, no_places=False, a=None):
        par = par or _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
        fpar = fpar or fit_flux_params()
        a = list(args if a is None else a)
        if no_places:
            a[5] = None
        _lib.check(lib.dv_infer_fields_measure_fit(eng._h, *a, 9, C.byref(par), *fields_out, None, *map(ptr, cat),
                                                   None if no_params else C.byref(fpar), *map(ptr, ff if out is None else out)))

    P, pl, D = np.ones((3, 31, 31, 3), np.float32), np.zeros((3, 2), np.int32), np.zeros((2, 40, 40, 3))
    ff2 = five(3, 3)

    def scene(stamps=P, places=pl, fptr=(0, 2, 3), n=3, cs=31, nb=3, data=D, M=2, F=40, fpar=None, out=None, no_params=False):
        fpar = fpar or fit_flux_params()
        fptr = None if fptr is None else np.asarray(fptr, np.int64)
        _lib.check(lib.dv_scene_fit_flux(ctx._h, ptr(stamps), ptr(places),
                                         None if fptr is None else fptr.ctypes.data_as(C.POINTER(C.c_int64)), n, cs, nb, ptr(data),
                                         M, F, None if no_params else C.byref(fpar), *map(ptr, ff2 if out is None else out)))

    nan = float("nan")
    for call in (pipeline, scene):
        with pytest.raises(DvError, match="params must be given"):
            call(no_params=True)
        for fpar, msg in ((_lib.DvFitFluxParams(0.0, 1 << 20), "min_pivot"), (_lib.DvFitFluxParams(1.0, 1 << 20), "min_pivot"),
                          (_lib.DvFitFluxParams(nan, 1 << 20), "min_pivot"), (_lib.DvFitFluxParams(-1e-8, 1 << 20), "min_pivot"),
                          (_lib.DvFitFluxParams(1e-8, 0), "scratch_bytes"), (_lib.DvFitFluxParams(1e-8, -5), "scratch_bytes")):
            with pytest.raises(DvError, match=msg):
                call(fpar=fpar)
        for k in range(5):                                        # a missing output
            out = list(ff if call is pipeline else ff2)
            out[k] = None
            with pytest.raises(DvError, match="must all be given"):
                call(out=out)
    # the pipeline: a null places in both forms, the two field-size refusals, what dv_infer_fields_measure refuses
    with pytest.raises(DvError, match="places"):
        pipeline(no_places=True)
    with pytest.raises(DvError, match="places"):
        pipeline(no_places=True, fields_out=(_dp(mean_f), _dp(std_f), None))
    with pytest.raises(DvError, match=rf"field 0 has 5 galaxies.*{NB * 25 * 8} bytes of scratch"):
        pipeline(fpar=_lib.DvFitFluxParams(1e-8, NB * 25 * 8 - 1))
    many = 1025
    _, _, big_args = Engine._field_args(fields, np.zeros((many, 2), np.int32), [0, many], np.zeros((many, 2), np.int32))
    with pytest.raises(DvError, match="field 0 has 1025 galaxies, the dense fit takes at most 1024"):
        pipeline(a=big_args)
    for par, msg in ((_lib.DvMeasureParams(NB, 3.0, 1e-10, 200), "band"), (_lib.DvMeasureParams(2, 0.0, 1e-10, 200), "sigma0"),
                     (_lib.DvMeasureParams(2, 3.0, 0.0, 200), "tol"), (_lib.DvMeasureParams(2, 3.0, 1e-10, -1), "max_iter")):
        with pytest.raises(DvError, match=msg):
            pipeline(par=par)
    with pytest.raises(DvError, match="go together"):
        pipeline(fields_out=(_dp(mean_f), None, None))
    # the host call: its inputs, the field table, the placements, the sizes
    for kw, msg in ((dict(stamps=None), "must all be given"), (dict(places=None), "must all be given"),
                    (dict(data=None), "must all be given"), (dict(fptr=None), "must all be given"),
                    (dict(fptr=(1, 2, 3)), "field_ptr must run from 0"), (dict(fptr=(0, 2, 4)), "field_ptr must run from 0"),
                    (dict(fptr=(0, 4, 3)), "decreases at field 1"), (dict(fptr=(0, -1, 3)), "decreases at field 0"),
                    (dict(places=np.array([[0, 0], [1 << 29, 0], [0, 0]], np.int32)), "placement 1"),
                    (dict(places=np.array([[0, 0], [0, 0], [0, -(1 << 29)]], np.int32)), "placement 2"),
                    (dict(F=0), "fields of 0 pixels"), (dict(F=40000), "fields of 40000 pixels"),
                    (dict(cs=0), "stamps of 0 pixels"), (dict(nb=17), "17 bands"), (dict(nb=0), "0 bands"),
                    (dict(fpar=_lib.DvFitFluxParams(1e-8, 3 * 4 * 8 - 1)), "field 0 has 2 galaxies")):
        with pytest.raises(DvError, match=msg):
            scene(**kw)
    # nothing to do with N = 0; the smallest scratch that takes the larger field runs
    scene(n=0, fptr=(0, 0, 0), stamps=None, places=None, out=[None] * 5)
    scene(fpar=_lib.DvFitFluxParams(1e-8, 3 * 4 * 8))
    # (two identical stamps of ones at one place and a third in a field of its own: the later twin is dropped and keeps
    # amplitude 1, which the first must undo on a field of zeros and has nothing to add to on a field of ones)
    assert ff2[4].tolist() == [[0] * 3, [5] * 3, [0] * 3] and (ff2[2] == 961.0).all() and (ff2[3] == 0.0).all()
    assert np.allclose(ff2[0], [[-1.0] * 3, [1.0] * 3, [0.0] * 3], rtol=0, atol=1e-12) and (ff2[0][1] == 1.0).all()
    scene(data=np.ones((2, 40, 40, 3)))
    assert ff2[4].tolist() == [[0] * 3, [5] * 3, [0] * 3] and (ff2[3] == 961.0).all()
    assert np.allclose(ff2[0], [[0.0] * 3, [1.0] * 3, [1.0] * 3], rtol=0, atol=1e-12) and np.isnan(ff2[1][1]).all()
    # the engine completes a correct call afterwards, with the bits it gave before
    again = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=3)
    for k in good:
        assert _eq(again[k], good[k]), k
    pipeline(fields_out=(_dp(mean_f), _dp(std_f), _dp(res_f)))
    assert np.array_equal(mean_f, eng.infer_fields_composite(fields, starts, places, fp, seed=9)["mean_fields"])
    ref = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=9)
    assert all(_eq(a, ref[k]) for a, k in zip(ff, KEYS))
