"""The non-negative flux fit on the GPU (dv_scene_fit_flux_nonneg, dv_infer_fields_measure_fit_nonneg,
DeblendFieldBatch(fit_flux=True, fit_nonneg=True)).  The kernel iterates on an active set, and a set
membership is a discontinuous function of the amplitudes: a comparison with another implementation is only meaningful where
rounding cannot move one.  So every comparison is made on a reference that first passes three assertions in numpy - conditions
of the bounds below, not measurements: the scaled condition number of every kept system is below 100; every passive galaxy has
a_i sqrt(G_ii) >= 1e-8 max |a sqrt(G)|; every clamped galaxy has y_i / sqrt(G_ii) >= 1e-8 max |h' / sqrt(G)|.  Rounding is of
order cond n 2^-53 = 1e-12 relative here, four orders below the margins.  With them: the clamped set, the statuses, the NaN
patterns and the iteration counts are equal exactly; on the final passive set section 7q's bounds hold - backward error 1e-10,
fit_scale within 1e-10 max|a| of numpy.linalg.solve, fit_var and sky_cov within 1e-9 relative of numpy.linalg.inv -; fit_dual
lies within 1e-10 (sum |G_ij a_j| + |h'_i|) of the same sum in numpy (at most 1027 terms times 2^-53 is 1.2e-13); fit_chi2
within the bound of the weighted test.  The worst fraction of each bound is printed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import fit_flux_nonneg_oracle as fn
from tests import fit_flux_oracle as fo
from tests import fit_flux_sky_oracle as fs
from tests import fit_flux_weighted_oracle as fw
from tests.test_fit_flux_nonneg_host import blob_scene
from tests.test_gpu_aperture import CAT, COUNTS, CS, NB, _blob_fields, _net, _windows
from tests.test_gpu_fit_flux import F2, _ctx, _eq
from tests.test_gpu_fit_flux import _scene as _scene71
from tests.test_gpu_fit_flux_sky import _check_solve

pytestmark = pytest.mark.gpu

KEYS = ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status")
WKEYS = KEYS + ("fit_chi2", "fit_npix")
SKY = ("sky_coef", "sky_cov", "sky_status", "sky_npix")
NN = ("fit_scale_free", "fit_clamped", "fit_dual")
NNF = ("nonneg_iters", "nonneg_status")
SHAPES = [(15, 3, 64), (31, 6, 97)]
CASES = [(cs, nb, F, order, weighted) for cs, nb, F in SHAPES for order in (None, 0, 1) for weighted in (False, True)]
NBLOB = 40


def _keys(order, weighted):
    return (WKEYS if weighted else KEYS) + (() if order is None else SKY) + NN + NNF


@functools.lru_cache(maxsize=None)
def _scene(cs, nb, F):
    """Six fields, 110 galaxies: (names, stamps, places, field_ptr, D, W); never written to.  Field 0: 40 random blobs, a third
    of them left out of D (noise 0.02).  Field 1: 40 other blobs, all of them in D - the all-positive field.  Field 2: the crowd
    of section 7l with its duplicate, its all-zero stamp and its two stamps outside; the duplicate keeps amplitude 1, so the
    galaxy it copies, in D at 0.6, is left with -0.4: a duplicate behind a clamped galaxy.  Field 3: no stamps.  Fields 4 and 5:
    one galaxy over a corner, one at an edge.  W: uniform(0.25, 4) inverse variances with a masked patch in every field, NaN
    in D2 (the data of the weighted calls) under it."""
    names71, s71, p71, fp71, _ = _scene71(cs, nb, F)
    crowd = slice(int(fp71[3]), int(fp71[4]))
    lone = [names71.index("alone corner"), names71.index("alone edge")]
    a0, pa0, D0 = blob_scene(NBLOB, cs, F, nb, 100 + cs)
    a1, pa1, D1 = blob_scene(NBLOB, cs, F, nb, 200 + cs, spurious=0)
    names = ["missing third"] * NBLOB + ["positive"] * NBLOB + names71[crowd] + ["alone corner", "alone edge"]
    stamps = np.concatenate([a0, a1, s71[crowd], s71[lone]])
    places = np.concatenate([pa0, pa1, p71[crowd], p71[lone]]).astype(np.int32)
    nc = crowd.stop - crowd.start
    fp = np.cumsum([0, NBLOB, NBLOB, nc, 0, 1, 1]).astype(np.int64)
    rng = np.random.default_rng(300 + cs)
    amps = rng.uniform(0.7, 1.3, size=len(names))
    amps[2 * NBLOB + names71[crowd].index("pair b")] = 0.6
    amps[2 * NBLOB + names71[crowd].index("duplicate")] = 0.0          # (a detection twice, one source)
    D = np.zeros((6, F, F, nb))
    D[0], D[1] = D0, D1
    for m in (2, 4, 5):
        for i in range(int(fp[m]), int(fp[m + 1])):
            ra, rz, ca, cz = fo.clip(places[i], cs, F)
            if rz > ra and cz > ca:
                pr, pc = places[i]
                D[m, ra:rz, ca:cz] += amps[i] * stamps[i, ra - pr:rz - pr, ca - pc:cz - pc].astype(np.float64)
    D[2:] += rng.normal(0.0, 0.02, size=D[2:].shape)
    W = rng.uniform(0.25, 4.0, size=D.shape)
    W[:, F // 3:F // 3 + cs // 2, F // 2:F // 2 + cs // 2] = 0.0
    D2 = D.copy()
    D2[W == 0.0] = np.nan
    for a in (stamps, places, fp, D, D2, W):
        a.flags.writeable = False
    return names, stamps, places, fp, D, D2, W


@functools.lru_cache(maxsize=None)
def _step1(cs, nb, F, weighted):
    _, stamps, places, fp, D, D2, W = _scene(cs, nb, F)
    return (fw.fit_flux(stamps, places, fp, D2, W) if weighted else fo.fit_flux(stamps, places, fp, D))[1]


def assert_margins(fields, fp, tag):
    """the three conditions of the module docstring, on the restatement's solves; returns what it met"""
    conds, passive, clamped = [], [], []
    for m, f in enumerate(fields):
        for s in f["bands"]:
            c, p, z = fn.margins(s, int(fp[m + 1] - fp[m]))
            conds.append(c), passive.append(p), clamped.append(z)
    print(f"{tag}: scaled condition up to {max(conds):.1f}, margins passive {min(passive):.1e} clamped {min(clamped):.1e}")
    assert max(conds) < 100.0 and min(passive) >= 1e-8 and min(clamped) >= 1e-8
    return max(conds), min(passive), min(clamped)


@functools.lru_cache(maxsize=None)
def _ref(cs, nb, F, order, weighted):
    """the restatement of the scene, computed once"""
    _, stamps, places, fp, D, D2, W = _scene(cs, nb, F)
    out, fields = fn.fit_flux_nonneg(stamps, places, fp, D2 if weighted else D, order, W if weighted else None,
                                     step1=_step1(cs, nb, F, weighted))
    for a in out.values():
        a.flags.writeable = False
    return out, fields


@functools.lru_cache(maxsize=None)
def _gpu(cs, nb, F, order, weighted):
    _, stamps, places, fp, D, D2, W = _scene(cs, nb, F)
    out = _ctx().scene_fit_flux_nonneg(stamps, places, D2 if weighted else D, field_ptr=fp, sky_order=order,
                                       weight_fields=W if weighted else None)
    for a in out.values():
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def _free(cs, nb, F, order, weighted):
    """the GPU's own call without the constraint"""
    _, stamps, places, fp, D, D2, W = _scene(cs, nb, F)
    if order is None:
        out = _ctx().scene_fit_flux(stamps, places, D2 if weighted else D, field_ptr=fp, weight_fields=W if weighted else None)
    else:
        out = _ctx().scene_fit_flux_sky(stamps, places, D2 if weighted else D, field_ptr=fp, sky_order=order,
                                        weight_fields=W if weighted else None)
    for a in out.values():
        a.flags.writeable = False
    return out


def _check_band(s, n, x, v, cov_sky, dual, worst):
    """one band of one field on the restatement's solve `s`: the GPU's unknowns x, variances v and sky covariance on the final
    passive set against numpy, and its duals against the same sum in numpy on its own amplitudes"""
    P = s["passive"]
    hp = np.zeros(len(x))
    hp[s["kept"]] = s["hp"]
    _check_solve(None, s["full"], None, dict(kept=P, hp=hp[P]), n, x, v, cov_sky, worst)
    for i in np.flatnonzero(s["clamped"]):
        terms = s["full"][i, P] * x[P]
        want, bound = terms.sum() - hp[i], 1e-10 * (np.abs(terms).sum() + abs(hp[i]))
        assert abs(dual[i] - want) <= bound, (i, dual[i], want)
        worst["dual"] = max(worst["dual"], abs(dual[i] - want) / bound)


@pytest.mark.parametrize("cs,nb,F,order,weighted", CASES)
def test_nonneg_fit_against_the_restatement(cs, nb, F, order, weighted):
    names, stamps, places, fp, D, D2, W = _scene(cs, nb, F)
    assert len(names) == 110 and np.diff(fp).tolist() == [NBLOB, NBLOB, 28, 0, 1, 1]
    q = 0 if order is None else fs.sky_terms(order)
    ref, fields = _ref(cs, nb, F, order, weighted)
    tag = f"{cs}/{nb}/{F} order {order} {'weighted' if weighted else 'unweighted'}"
    assert_margins(fields, fp, tag)
    # the reference does what the test is about: clamping in fields 0 and 2, none in field 1, several iterations, convergence
    assert (ref["nonneg_status"] == 0).all() and (ref["nonneg_iters"][1] == 1).all() and ref["nonneg_iters"][0].min() >= 2
    assert (ref["nonneg_iters"][3] == (1 if q else 0)).all() and ref["nonneg_iters"].max() <= 8
    assert ref["fit_clamped"][:NBLOB].sum() >= 4 * nb and ref["fit_clamped"][NBLOB:2 * NBLOB].sum() == 0
    first_b = 2 * NBLOB + names[2 * NBLOB:].index("pair b")
    assert (ref["fit_clamped"][first_b] == 1).all() and (ref["fit_status"][names.index("duplicate")] == 5).all()
    assert (ref["fit_status"][names.index("zero")] == 4).all()
    print(f"{tag}: {int(ref['fit_clamped'].sum())} clamped of {ref['fit_clamped'].size}, nonneg_iters "
          f"{np.bincount(ref['nonneg_iters'].ravel()).tolist()}")

    got = _gpu(cs, nb, F, order, weighted)
    M = len(fp) - 1
    assert list(got) == list(_keys(order, weighted))
    assert got["fit_clamped"].dtype == np.int32 and got["nonneg_iters"].dtype == np.int32 and got["nonneg_iters"].shape == (M, nb)
    # the sets, the statuses, the NaN patterns and the iterations, exactly
    for k in ("fit_clamped", "fit_status", "nonneg_iters", "nonneg_status") + (("fit_npix",) if weighted else ()) + \
            (("sky_status", "sky_npix") if q else ()):
        assert np.array_equal(got[k], ref[k]), k
    for k in ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_scale_free", "fit_dual") + (("fit_chi2",) if weighted else ()) + \
            (("sky_coef", "sky_cov") if q else ()):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
    z = got["fit_clamped"] == 1
    assert (got["fit_scale"][z] == 0.0).all() and not np.signbit(got["fit_scale"][z]).any() and np.isnan(got["fit_var"][z]).all()
    ok = got["fit_status"] == 0
    assert (got["fit_scale"][ok] >= 0.0).all() and (got["fit_dual"][ok] >= 0.0).all() and (got["fit_dual"][ok & ~z] == 0.0).all()
    assert (got["fit_scale_free"][z] < 0.0).any() and np.isnan(got["fit_dual"][~ok]).all()
    assert (got["fit_scale"][got["fit_status"] == 5] == 1.0).all()
    # what iteration 1 fixes has the bits of the GPU's own call without the constraint
    free = _free(cs, nb, F, order, weighted)
    assert _eq(got["fit_scale_free"], free["fit_scale"])
    for k in ("fit_gram", "fit_proj", "fit_status") + (("fit_npix",) if weighted else ()) + (("sky_npix", "sky_status") if q else ()):
        assert _eq(got[k], free[k]), k
    worst = dict(backward=0.0, solve=0.0, var=0.0, cov=0.0, dual=0.0)
    for m, f in enumerate(fields):
        lo, hi = int(fp[m]), int(fp[m + 1])
        n = hi - lo
        for b, s in enumerate(f["bands"]):
            sky_x = got["sky_coef"][m, b] if q else np.zeros(0)
            sky_c = got["sky_cov"][m, b] if q else np.zeros((0, 0))
            x = np.concatenate([got["fit_scale"][lo:hi, b], sky_x])
            v = np.concatenate([got["fit_var"][lo:hi, b], np.diagonal(sky_c)])
            dual = np.concatenate([got["fit_dual"][lo:hi, b], np.zeros(q)])
            _check_band(s, n, x, v, sky_c, dual, worst)
    if weighted:
        for m in range(M):
            lo, hi = int(fp[m]), int(fp[m + 1])
            coef = got["sky_coef"][m] if q else np.zeros((nb, 0))
            stat = got["sky_status"][m] if q else np.zeros((nb, 0), np.int32)
            chi2, npix, yard = fs.chi2_field(stamps[lo:hi], np.asarray(places[lo:hi], np.int64), D2[m], W[m], got["fit_scale"][lo:hi],
                                             got["fit_status"][lo:hi], coef, stat)
            assert np.array_equal(got["fit_npix"][lo:hi], npix) and np.array_equal(np.isnan(got["fit_chi2"][lo:hi]), np.isnan(chi2))
            fin = ~np.isnan(chi2)
            err = np.abs(got["fit_chi2"][lo:hi][fin] - chi2[fin])
            assert (err <= 1e-12 * yard[fin]).all(), (m, float((err / yard[fin]).max()))
            if fin.any():
                worst["chi2"] = max(worst.get("chi2", 0.0), float((err / np.where(yard[fin] > 0, yard[fin], 1.0)).max() / 1e-12))
    print(f"{tag}: worst fraction of each bound - " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def _grid_scene(n, cs, step, per_row, F, seed):
    """n stamps of cs px on a grid of `step` px, one band; every third one is left out of D; noise 0.05"""
    rng = np.random.default_rng(seed)
    cells = np.arange(n)
    places = np.stack([(cells // per_row) * step, (cells % per_row) * step], axis=1).astype(np.int32)
    stamps = np.stack([fo.elliptical_gaussian(cs, (0.35 * cs / 3, rng.uniform(-0.05, 0.05) * cs, 0.35 * cs / 3),
                                              rng.uniform(-0.3, 0.3, 2), rng.uniform(0.5, 2.0)) for _ in range(n)])[..., None]
    stamps = stamps.astype(np.float32)
    D = rng.normal(0.0, 0.05, size=(1, F, F, 1))
    for i in range(n):
        if i % 3 == 2:
            continue
        ra, rz, ca, cz = fo.clip(places[i], cs, F)
        D[0, ra:rz, ca:cz] += stamps[i, ra - places[i, 0]:rz - places[i, 0], ca - places[i, 1]:cz - places[i, 1]].astype(np.float64)
    return stamps, places, D


@pytest.mark.parametrize("n,cs,step,per_row,F", [(300, 9, 3, 18, 64), (1024, 3, 2, 32, 67)])
@pytest.mark.parametrize("order", [None, 1])
def test_more_unknowns_than_threads_and_the_largest_system(n, cs, step, per_row, F, order):
    """300 stamps of 9 px (every 64- or 256-strided loop of the kernel takes several turns) and exactly 1024 stamps of 3 px
    (with the plane 1027 unknowns, the largest system), a third of them without a source, against numpy on the GPU's own
    matrix"""
    stamps, places, D = _grid_scene(n, cs, step, per_row, F, seed=9 + n)
    ctx = _ctx()
    if order is None:
        g = ctx.scene_fit_flux_gram(stamps, places, D[0])
        A, rhs = g["gram"][0], g["proj"][:, 0]
    else:
        g = ctx.scene_fit_flux_sky_gram(stamps, places, D[0], sky_order=order)
        A, rhs = g["gram"][0], g["rhs"][:, 0]
    q = A.shape[0] - n
    s = fn.solve_band_nonneg(A, rhs, n, fast=True)
    tag = f"{n} x {cs} px order {order}"
    assert_margins([dict(bands=[s])], [0, n], tag)
    assert s["nn_status"] == 0 and 2 <= s["iters"] <= 8 and s["clamped"].sum() >= n // 10
    print(f"{tag}: {int(s['clamped'].sum())} clamped, {s['iters']} factorisations, |V| {s['sizes']}")
    got = ctx.scene_fit_flux_nonneg(stamps, places, D, sky_order=order)
    assert (got["fit_status"] == 0).all() and got["nonneg_status"][0, 0] == 0
    assert np.array_equal(got["fit_clamped"][:, 0], s["clamped"][:n]) and got["nonneg_iters"][0, 0] == s["iters"]
    z = got["fit_clamped"][:, 0] == 1
    assert (got["fit_scale"][z, 0] == 0.0).all() and np.isnan(got["fit_var"][z, 0]).all() and (got["fit_scale"][~z, 0] > 0.0).all()
    assert (got["fit_dual"][z, 0] > 0.0).all() and (got["fit_dual"][~z, 0] == 0.0).all()
    sky_x = got["sky_coef"][0, 0] if q else np.zeros(0)
    sky_c = got["sky_cov"][0, 0] if q else np.zeros((0, 0))
    worst = dict(backward=0.0, solve=0.0, var=0.0, cov=0.0, dual=0.0)
    _check_band(s, n, np.concatenate([got["fit_scale"][:, 0], sky_x]), np.concatenate([got["fit_var"][:, 0], np.diagonal(sky_c)]),
                sky_c, np.concatenate([got["fit_dual"][:, 0], np.zeros(q)]), worst)
    print(f"{tag}: worst fraction of each bound - " + ", ".join(f"{k} {w:.1e}" for k, w in worst.items()))
    free = ctx.scene_fit_flux(stamps, places, D) if order is None else ctx.scene_fit_flux_sky(stamps, places, D, sky_order=order)
    assert _eq(got["fit_scale_free"], free["fit_scale"]) and (free["fit_scale"] < 0.0).sum() >= n // 10
    for k in ("fit_status", "fit_gram", "fit_proj"):
        assert _eq(got[k], free[k]), k


@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_rows_and_fields_keep_their_bits(cs, nb, F):
    _, stamps, places, fp, D, D2, W = _scene(cs, nb, F)
    ctx = _ctx()
    M = len(fp) - 1
    pos = slice(int(fp[1]), int(fp[2]))
    for order, weighted in ((None, False), (1, True), (0, False), (None, True)):
        keys = _keys(order, weighted)
        got = _gpu(cs, nb, F, order, weighted)
        Dm, Wm = (D2, W) if weighted else (D, None)
        # the all-positive field: one factorisation, and every shared array has the bits of the call without the constraint
        free = _free(cs, nb, F, order, weighted)
        assert (got["nonneg_iters"][1] == 1).all() and (got["fit_clamped"][pos] == 0).all() and (got["fit_dual"][pos] == 0.0).all()
        for k in (WKEYS if weighted else KEYS):
            assert _eq(got[k][pos], free[k][pos]), k
        for k in (SKY if order is not None else ()):
            assert _eq(got[k][1], free[k][1]), k
        call = lambda s, p, d, **kw: ctx.scene_fit_flux_nonneg(s, p, d, sky_order=order, **kw)     # noqa: E731
        again = call(stamps, places, Dm, field_ptr=fp, weight_fields=Wm)
        for k in keys:
            assert _eq(again[k], got[k]), k
        # the fields and the weights in reverse order
        order_r = np.concatenate([np.arange(fp[m], fp[m + 1]) for m in range(M - 1, -1, -1)])
        fp_r = np.concatenate([[0], np.cumsum(np.diff(fp)[::-1])])
        moved = call(stamps[order_r], places[order_r], Dm[::-1], field_ptr=fp_r, weight_fields=None if Wm is None else Wm[::-1])
        for k in keys:
            assert _eq(moved[k], got[k][::-1] if k in SKY + NNF else got[k][order_r]), k
        # one field alone in the call - the field without galaxies too
        for m in (0, 2, 3):
            lo, hi = int(fp[m]), int(fp[m + 1])
            one = call(stamps[lo:hi], places[lo:hi], Dm[m:m + 1], weight_fields=None if Wm is None else Wm[m])
            for k in keys:
                assert _eq(one[k], got[k][m:m + 1] if k in SKY + NNF else got[k][lo:hi]), (m, k)
        # a scratch that holds the largest field's matrices and no more: three sub-ranges
        q = 0 if order is None else fs.sky_terms(order)
        split = call(stamps, places, Dm, field_ptr=fp, weight_fields=Wm, scratch_bytes=nb * (NBLOB + q) * (NBLOB + q) * 8)
        for k in keys:
            assert _eq(split[k], got[k]), k
    # the iteration cap: one factorisation is the call without the constraint, flagged
    capped = ctx.scene_fit_flux_nonneg(stamps, places, D, field_ptr=fp, max_iter=1)
    free = _free(cs, nb, F, None, False)
    for k in KEYS:
        assert _eq(capped[k], free[k]), k
    assert (capped["fit_clamped"] == 0).all() and (capped["nonneg_iters"] == [[1], [1], [1], [0], [1], [1]]).all()
    assert capped["nonneg_status"][:, 0].tolist() == [1, 0, 1, 0, 0, 0]


def _pipeline_fields(eng, starts, places, fp):
    """the source fields of the pipeline tests: blob fields less 0.5 x every third mean stamp the network returns for them, so
    that the refit of the network's stamps to the changed fields wants negative amplitudes"""
    fields = _blob_fields(5, F2, seed=11)
    first = eng.infer_fields_keep(fields, starts, fp, seed=77)["loc"]
    for m in range(5):
        for i in range(int(fp[m]), int(fp[m + 1])):
            if i % 3 == 0:
                ra, rz, ca, cz = fo.clip(places[i], CS, F2)
                pr, pc = places[i]
                fields[m, ra:rz, ca:cz] -= 0.5 * first[i, ra - pr:rz - pr, ca - pc:cz - pc].astype(np.float64)
    return fields


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_host_call(dtype, monkeypatch):
    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    starts, places, fp = _windows(F2, COUNTS, seed=5)
    fields = _pipeline_fields(eng, starts, places, fp)
    rng = np.random.default_rng(7100 + CS)
    W = rng.uniform(0.25, 4.0, size=fields.shape)
    W[:, F2 // 3:F2 // 3 + CS // 2, F2 // 2:F2 // 2 + CS // 2] = 0.0
    seed = 77
    stamps = eng.infer_fields_keep(fields, starts, fp, seed=seed)["loc"]
    rows = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    fb = F2 * F2 * NB * 8
    # (the group sizes of tests/test_gpu_fit_flux_sky.py: three resident fields, so that field 2 is carried across groups)
    assert 3 * 4 * fb <= 10 << 20 < 4 * 4 * fb and 3 * 5 * fb <= 13 << 20 < 4 * 5 * fb
    assert 3 * fb <= 3 << 20 < 4 * fb and 3 * 2 * fb <= 5 << 20 < 4 * 2 * fb
    for order, weights, mb_fields, mb_only in ((None, None, "10", "3"), (1, None, "10", "3"), (0, W, "13", "5")):
        keys = _keys(order, weights is not None)
        want = ctx.scene_fit_flux_nonneg(stamps, places, fields, field_ptr=fp, sky_order=order, weight_fields=weights)
        assert want["fit_clamped"].sum() > 0 and (want["nonneg_iters"] > 1).any() and (want["nonneg_status"] == 0).all()
        assert (want["nonneg_iters"][1] == (0 if order is None else 1)).all()          # the field without stamps
        got = eng.infer_fields_measure_fit_nonneg(fields, starts, fp, places, order, weights, seed=seed)
        assert sorted(got) == sorted(tuple(rows) + keys)
        for k in keys:
            assert _eq(got[k], want[k]), k
        for k in rows:                                            # every shared output has infer_fields_measure's bits
            assert _eq(got[k], rows[k]), k
        only = eng.infer_fields_measure_fit_nonneg(fields, starts, fp, places, order, weights, seed=seed, return_fields=False)
        assert sorted(only) == sorted(CAT + ("mse_center",) + keys)
        for k in only:
            assert _eq(only[k], got[k]), k
        monkeypatch.setenv("DV_FIELDS_GROUP_MB", mb_fields)
        grouped = eng.infer_fields_measure_fit_nonneg(fields, starts, fp, places, order, weights, seed=seed)
        for k in got:
            assert _eq(grouped[k], got[k]), k
        monkeypatch.setenv("DV_FIELDS_GROUP_MB", mb_only)
        g2 = eng.infer_fields_measure_fit_nonneg(fields, starts, fp, places, order, weights, seed=seed, return_fields=False)
        for k in only:
            assert _eq(g2[k], only[k]), k
        monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    # the calls without the constraint beside it are what they were; M = 1 is the single-field view
    plain = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=seed, return_fields=False)
    w0 = ctx.scene_fit_flux(stamps, places, fields, field_ptr=fp)
    assert all(_eq(plain[k], w0[k]) for k in KEYS) and "fit_clamped" not in plain
    m = 3
    s1, p1 = starts[fp[m]:fp[m + 1]], places[fp[m]:fp[m + 1]]
    one = eng.infer_cutouts_measure_fit_nonneg(fields[m], s1, p1, 1, W[m], seed=seed)
    st1 = eng.infer_fields_keep(fields[m:m + 1], s1, [0, len(s1)], seed=seed)["loc"]
    w1 = ctx.scene_fit_flux_nonneg(st1, p1, fields[m:m + 1], sky_order=1, weight_fields=W[m])
    assert "mean_field" in one and all(_eq(one[k], w1[k]) for k in _keys(1, True))
    # a call whose fields hold no stamp at all: the sky is fitted in one factorisation, without a sky there is none
    for order in (1, None):
        none = eng.infer_fields_measure_fit_nonneg(fields[:2], np.zeros((0, 2), np.int32), [0, 0, 0], np.zeros((0, 2), np.int32),
                                                   order, seed=seed, return_fields=False)
        assert (none["nonneg_iters"] == (0 if order is None else 1)).all() and (none["nonneg_status"] == 0).all()


def test_deblend_field_batch_constrains_the_fit():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    rng = np.random.default_rng(4)
    dists = [rng.integers(-45, 46, size=(n, 2)).astype(np.float64) for n in (20, 0, 45)]
    places = np.concatenate([int((F2 - CS) / 2) + d.astype(np.int64) for d in dists])
    fp = np.cumsum([0, 20, 0, 45])
    net0 = _net("float32")
    eng0 = net0._core.engine
    fields = _blob_fields(3, F2, seed=21)
    first = eng0.infer_fields_keep(fields, places.astype(np.int32), fp, seed=1)["loc"]
    for m in range(3):
        for i in range(int(fp[m]), int(fp[m + 1])):
            if i % 3 == 0:
                pr, pc = places[i]
                fields[m, pr:pr + CS, pc:pc + CS] -= 0.5 * first[i].astype(np.float64)
    W = np.random.default_rng(7100 + CS).uniform(0.25, 4.0, size=fields.shape)
    W[:, F2 // 3:F2 // 3 + CS // 2, F2 // 2:F2 // 2 + CS // 2] = 0.0

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds
        return DeblendFieldBatch(net, fields, CS, NB)

    host_b = batch()
    host = host_b.deblend_fields(dists, measure=True)             # the default path: stamps and catalogue on the host
    plain = batch().deblend_fields(dists, on_device=True, measure=True)
    mean = np.concatenate([np.stack([np.asarray(x) for x in h["output_images_mean"]]) for h in host if len(h)])
    cat = np.recarray((int(fp[-1]),), dtype=[("flux", "<f8", (NB,))])
    cat["flux"] = np.concatenate([h["flux"] for h in host])
    for order, weights, sky_sigma in ((None, None, np.full(NB, 0.3)), (1, None, None), (0, W, None)):
        a = batch()
        res = a.deblend_fields(dists, on_device=True, measure=True, fit_flux=True, fit_nonneg=True, fit_sky=order,
                               fit_weights=weights, sky_sigma=sky_sigma)
        want, per_field = ms.fit_fluxes_nonneg(mean, places, fields, sky_order=order, weight_fields=weights, field_ptr=fp,
                                               catalogue=cat, sky_sigma=sky_sigma, ctx=host_b._ctx)
        assert want["fit_clamped"].sum() > 0                      # the scene does what the test is about
        fit_cols = DeblendFieldBatch.fit_flux_columns(NB) if weights is None else DeblendFieldBatch.fit_flux_weighted_columns(NB)
        want_cols = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + fit_cols +
                             ([] if order is None else DeblendFieldBatch.fit_sky_columns(NB)) +
                             DeblendFieldBatch.fit_nonneg_columns(NB))
        for k in NNF:
            assert _eq(a.nonneg_fit[k], per_field[k]), k          # the field without galaxies included
        assert (a.sky_fit is None) == (order is None)
        for m, (r, p) in enumerate(zip(res, plain)):
            assert r.dtype == want_cols and len(r) == len(p)
            for k in p.dtype.names:                               # the columns of the call without it, value for value
                if k != "shifts":
                    assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].base.kind == "f"), k
            for k in want.dtype.names:
                assert np.array_equal(r[k], want[k][fp[m]:fp[m + 1]], equal_nan=True), (m, k)
        cat_only = batch().deblend_fields(dists, on_device=True, measure=True, fit_flux=True, fit_nonneg=True, fit_sky=order,
                                          fit_weights=weights, sky_sigma=sky_sigma, return_fields=False)
        for r, c in zip(res, cat_only):
            for k in r.dtype.names:
                if k != "shifts":
                    assert np.array_equal(r[k], c[k], equal_nan=r.dtype[k].base.kind == "f"), k


def test_refusals_come_before_any_gpu_work_and_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import Engine, _dp, _fp, _ip, fit_flux_params

    DvError, lib = _lib.DvError, _lib.lib
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(1, F2, seed=11)
    starts, places, fp = _windows(F2, [5], seed=5, hang=False)
    W1 = np.random.default_rng(7100 + CS).uniform(0.25, 4.0, size=fields.shape)
    good = eng.infer_fields_measure_fit_nonneg(fields, starts, fp, places, 1, W1, seed=3)
    good0 = eng.infer_fields_measure_fit_nonneg(fields, starts, fp, places, seed=3)
    n, nb = 5, NB

    def ptr(a):
        if a is None:
            return None
        if a.dtype == np.int64:
            return a.ctypes.data_as(C.POINTER(C.c_int64))
        return _dp(a) if a.dtype == np.float64 else _fp(a) if a.dtype == np.float32 else _ip(a)

    cat = [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    seven = lambda n, nb: [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb), np.int32),   # noqa: E731
                           np.zeros((n, nb)), np.zeros((n, nb), np.int32)]
    four = lambda M, nb, q: [np.zeros((M, nb, q)), np.zeros((M, nb, q, q)), np.zeros((M, nb, q), np.int32), np.zeros((M, nb), np.int64)]   # noqa: E731
    five = lambda n, M, nb: [np.zeros((n, nb)), np.zeros((n, nb), np.int32), np.zeros((n, nb)), np.zeros((M, nb), np.int32),   # noqa: E731
                             np.zeros((M, nb), np.int32)]
    ff, sk, nn = seven(n, nb), four(1, nb, 3), five(n, 1, nb)
    f2, N, args = Engine._field_args(fields, starts, fp, places)

    def pipeline(fpar=None, out=None, sky=None, new=None, weights=W1, order=1, max_iter=100, no_params=False, a=None):
        par = _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
        fpar = fpar or fit_flux_params()
        if out is None:                                           # (the chi-square outputs are NULL exactly when the weights are)
            out = ff[:5] + ([None, None] if weights is None else ff[5:])
        if sky is None:                                           # (... and the sky outputs exactly when there is no sky)
            sky = [None] * 4 if order == -1 else sk
        _lib.check(lib.dv_infer_fields_measure_fit_nonneg(eng._h, *(args if a is None else a), 9, C.byref(par), None, None, None,
                                                          None, *map(ptr, cat), None if no_params else C.byref(fpar), ptr(weights),
                                                          order, max_iter, *map(ptr, out), *map(ptr, sky),
                                                          *map(ptr, nn if new is None else new)))

    P, pl, D = np.ones((3, 31, 31, 3), np.float32), np.zeros((3, 2), np.int32), np.zeros((2, 40, 40, 3))
    Wd = np.ones_like(D)
    ff2, sk2, nn2 = seven(3, 3), four(2, 3, 3), five(3, 2, 3)

    def scene(stamps=P, places=pl, fptr=(0, 2, 3), n=3, data=D, weights=Wd, fpar=None, out=None, sky=None, new=None, order=1,
              max_iter=100, no_params=False):
        fpar = fpar or fit_flux_params()
        fptr = np.asarray(fptr, np.int64)
        if out is None:
            out = ff2[:5] + ([None, None] if weights is None else ff2[5:])
        if sky is None:
            sky = [None] * 4 if order == -1 else sk2
        _lib.check(lib.dv_scene_fit_flux_nonneg(ctx._h, ptr(stamps), ptr(places), fptr.ctypes.data_as(C.POINTER(C.c_int64)), n, 31, 3,
                                                ptr(data), ptr(weights), len(fptr) - 1, 40, None if no_params else C.byref(fpar),
                                                order, max_iter, *map(ptr, out), *map(ptr, sky), *map(ptr, nn2 if new is None else new)))

    for call in (pipeline, scene):
        base, skb, nnb = (ff, sk, nn) if call is pipeline else (ff2, sk2, nn2)
        with pytest.raises(DvError, match="params must be given"):
            call(no_params=True)
        for max_iter in (0, -3):
            with pytest.raises(DvError, match="max_iter must be at least 1"):
                call(max_iter=max_iter)
            with pytest.raises(DvError, match="max_iter must be at least 1"):
                call(max_iter=max_iter, order=-1, weights=None)
        for order in (2, -2, 3):
            with pytest.raises(DvError, match="sky_order must be 0"):
                call(order=order)
        for k in range(4):                                        # a sky output given with sky_order -1
            sky = [None] * 4
            sky[k] = skb[k]
            with pytest.raises(DvError, match="sky_order -1 fits no sky"):
                call(order=-1, sky=sky)
        for k in range(5):                                        # a missing new output
            new = list(nnb)
            new[k] = None
            with pytest.raises(DvError, match="fit_scale_free, fit_clamped, fit_dual, nonneg_iters and nonneg_status must all be given"):
                call(new=new)
        # what the sky and weighted calls refuse
        for fpar, msg in ((_lib.DvFitFluxParams(0.0, 1 << 20), "min_pivot"), (_lib.DvFitFluxParams(1e-8, 0), "scratch_bytes")):
            with pytest.raises(DvError, match=msg):
                call(fpar=fpar)
        for k in range(7):                                        # a missing galaxy output, weighted
            out = list(base)
            out[k] = None
            with pytest.raises(DvError, match="must all be given"):
                call(out=out)
        for k in range(4):                                        # a missing sky output
            sky = list(skb)
            sky[k] = None
            with pytest.raises(DvError, match="sky_coef, sky_cov, sky_status and sky_npix must all be given"):
                call(sky=sky)
        for order in (1, -1):                                     # chi-square outputs without weights
            for k in (5, 6):
                out = list(base)
                out[k] = None
                with pytest.raises(DvError, match="without weight_fields both must be NULL"):
                    call(weights=None, out=out, order=order)
    with pytest.raises(DvError, match=rf"field 0 has 5 galaxies and 3 sky terms.*{NB * 64 * 8} bytes of scratch"):
        pipeline(fpar=_lib.DvFitFluxParams(1e-8, NB * 64 * 8 - 1))
    with pytest.raises(DvError, match=r"field 0 has 2 galaxies: its Gram matrices need 96 bytes of scratch"):
        scene(fpar=_lib.DvFitFluxParams(1e-8, 3 * 4 * 8 - 1), order=-1)
    many = 1025
    _, _, big_args = Engine._field_args(fields, np.zeros((many, 2), np.int32), [0, many], np.zeros((many, 2), np.int32))
    with pytest.raises(DvError, match="field 0 has 1025 galaxies, the dense fit takes at most 1024"):
        pipeline(a=big_args)
    chain = np.stack([np.zeros(many), (np.arange(many) % 3) * 30], axis=1).astype(np.int32)
    with pytest.raises(DvError, match="field 1 has 1025 galaxies, the dense fit takes at most 1024"):
        ctx.scene_fit_flux_nonneg(np.ones((1 + many, 31, 31, 3), np.float32), np.concatenate([pl[:1], chain]), D,
                                  field_ptr=[0, 1, 1 + many])
    # the smallest scratch that takes the larger field runs: two identical stamps of ones at one place and a third in a field of
    # its own, on fields of zeros under unit weights - the later twin is dropped and keeps amplitude 1, which the first would undo
    # with -1 and is clamped for; without a sky nothing else is left in the system, and the dual of the clamped twin is -h' = 961
    scene(fpar=_lib.DvFitFluxParams(1e-8, 3 * 4 * 8), order=-1)
    assert ff2[4].tolist() == [[0] * 3, [5] * 3, [0] * 3] and (ff2[2] == 961.0).all() and (ff2[6] == 961).all()
    assert (ff2[0][0] == 0.0).all() and (ff2[0][1] == 1.0).all() and np.abs(ff2[0][2]).max() < 1e-12
    assert np.allclose(nn2[0][0], -1.0, rtol=0, atol=1e-12) and nn2[1].tolist() == [[1] * 3, [0] * 3, [0] * 3]
    assert np.allclose(nn2[2][0], 961.0, rtol=1e-12) and np.isnan(nn2[2][1]).all() and (nn2[3] == [[2] * 3, [1] * 3]).all()
    assert (nn2[4] == 0).all() and (sk2[2] == 0).all()
    # the engine completes correct calls afterwards, with the bits it gave before
    again = eng.infer_fields_measure_fit_nonneg(fields, starts, fp, places, 1, W1, seed=3)
    for k in good:
        assert _eq(again[k], good[k]), k
    again0 = eng.infer_fields_measure_fit_nonneg(fields, starts, fp, places, seed=3)
    for k in good0:
        assert _eq(again0[k], good0[k]), k
    pipeline()
    ref = eng.infer_fields_measure_fit_nonneg(fields, starts, fp, places, 1, W1, seed=9, return_fields=False)
    assert all(_eq(a, ref[k]) for a, k in zip(ff + sk + nn, WKEYS + SKY + NN + NNF))
