"""The weighted flux fit on the GPU (dv_scene_fit_flux_weighted, dv_infer_fields_measure_fit_weighted,
DeblendFieldBatch(fit_flux=True, fit_weights=W)) on the 71-galaxy scene of tests/test_gpu_fit_flux.py under
random weights with masks.  Unit weights and powers of two against the unweighted call, bit for bit; steps 1 - 5 against the
numpy restatement of tests/fit_flux_weighted_oracle.py with the bounds of section 7q (their derivations hold with one more
rounding per term), valid where they were derived: the test first asserts, on the CPU, that every scaled Gram matrix has a
condition number below 100.  The chi-square is compared with the restatement evaluated on the GPU's own fit_scale and
fit_status, within 1e-12 sum W R^2, R = |D| + sum |a_j P_j|: M carries at most k + 1 roundings for k <= ~40 neighbours, r one
more, the two products two, and the sum at most npix 2^-53 - about (45 + 3481) 1.1e-16 = 4e-13 of that yardstick at the very
most.  Then the pipeline stage against the host call, bit for bit, on both engines."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import fit_flux_oracle as fo
from tests import fit_flux_weighted_oracle as fw
from tests.test_gpu_aperture import CAT, COUNTS, CS, NB, _blob_fields, _net, _windows
from tests.test_gpu_fit_flux import F2, NBIG, SHAPES, _ctx, _eq, _gpu, _scene

pytestmark = pytest.mark.gpu

KEYS = ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status")
WKEYS = KEYS + ("fit_chi2", "fit_npix")


def _draw_weights(rng, shape, cs):
    """uniform(0.25, 4) inverse variances, a tenth of the entries masked, and a masked block (fields first: (M, F, F, nb))"""
    F = shape[1]
    W = rng.uniform(0.25, 4.0, size=shape)
    W[rng.random(shape) < 0.1] = 0.0
    W[:, F // 3:F // 3 + cs // 4, F // 2:F // 2 + cs // 3] = 0.0
    return W


def _spoil(rng, W, D):
    """a handful of the masked entries rewritten as NaN, -1 and inf, and NaN written into D under some masked pixels: no
    counting pixel changes"""
    W, D = W.copy(), D.copy()
    at = np.flatnonzero(W.ravel() == 0.0)
    pick = rng.choice(at, size=min(60, at.size), replace=False)
    W.ravel()[pick] = np.resize([np.nan, -1.0, np.inf], pick.size)
    D.ravel()[rng.choice(at, size=min(200, at.size), replace=False)] = np.nan
    return W, D


@functools.lru_cache(maxsize=None)
def _wscene(cs, nb, F):
    """(names, stamps, places, field_ptr, D with NaN under some masks, W, W before the non-finite rewrites); never written to"""
    names, stamps, places, fp, D = _scene(cs, nb, F)
    rng = np.random.default_rng(7100 + cs)
    clean = _draw_weights(rng, D.shape, cs)
    W, Dn = _spoil(rng, clean, D)
    for a in (W, Dn, clean):
        a.flags.writeable = False
    return names, stamps, places, fp, Dn, W, clean


@functools.lru_cache(maxsize=None)
def _wref(cs, nb, F):
    """the restatement of the weighted scene, computed once"""
    _, stamps, places, fp, D, W, _ = _wscene(cs, nb, F)
    out, fields = fw.fit_flux(stamps, places, fp, D, W)
    for a in out.values():
        a.flags.writeable = False
    return out, fields


@functools.lru_cache(maxsize=None)
def _wgpu(cs, nb, F):
    _, stamps, places, fp, D, W, _ = _wscene(cs, nb, F)
    out = _ctx().scene_fit_flux(stamps, places, D, field_ptr=fp, weight_fields=W)
    for a in out.values():
        a.flags.writeable = False
    return out


@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_unit_weights_and_powers_of_two(cs, nb, F):
    _, stamps, places, fp, D = _scene(cs, nb, F)
    plain = _gpu(cs, nb, F)
    ones = _ctx().scene_fit_flux(stamps, places, D, field_ptr=fp, weight_fields=np.ones_like(D))
    assert sorted(ones) == sorted(WKEYS) and ones["fit_chi2"].shape == (71, nb) and ones["fit_npix"].dtype == np.int32
    for k in KEYS:
        assert _eq(ones[k], plain[k]), k
    # every pixel of the clipped stamp counts
    area = np.array([max(0, min(p[0] + cs, F) - max(p[0], 0)) * max(0, min(p[1] + cs, F) - max(p[1], 0)) for p in places])
    assert np.array_equal(ones["fit_npix"], np.repeat(area[:, None], nb, axis=1))
    assert np.array_equal(np.isnan(ones["fit_chi2"]), plain["fit_status"] == 4)
    quarter = _ctx().scene_fit_flux(stamps, places, D, field_ptr=fp, weight_fields=np.full_like(D, 0.25))
    assert _eq(quarter["fit_scale"], plain["fit_scale"]) and _eq(quarter["fit_status"], plain["fit_status"])
    assert _eq(quarter["fit_var"], 4.0 * plain["fit_var"])
    assert _eq(quarter["fit_gram"], 0.25 * plain["fit_gram"]) and _eq(quarter["fit_proj"], 0.25 * plain["fit_proj"])
    assert _eq(quarter["fit_chi2"], 0.25 * ones["fit_chi2"]) and _eq(quarter["fit_npix"], ones["fit_npix"])


@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_weighted_fit_against_the_restatement(cs, nb, F):
    names, stamps, places, fp, D, W, clean = _wscene(cs, nb, F)
    with np.errstate(invalid="ignore"):
        assert np.isnan(D).any() and np.isnan(W).any() and np.isinf(W).any() and (W < 0).any()
    assert np.array_equal(fw.counts(W), clean > 0)                 # the rewrites change no counting pixel
    ref, fields = _wref(cs, nb, F)
    conds = [fo.scaled_condition(s["full"], s["kept"]) for f in fields for s in f["bands"]]
    counts = np.bincount(ref["fit_status"].ravel(), minlength=6)
    print(f"{cs}/{nb}/{F}: worst scaled condition {max(conds):.1f}, status 5: {counts[5]}, status 4: {counts[4]}")
    assert max(conds) < 100.0
    assert counts[5] == nb and counts[4] == 3 * nb                 # the duplicate; the zero stamp and the two outside: no mask adds any
    got = _wgpu(cs, nb, F)
    assert sorted(got) == sorted(WKEYS) and all(got[k].shape == (71, nb) for k in WKEYS)
    assert got["fit_status"].dtype == np.int32 and got["fit_npix"].dtype == np.int32
    # the statuses, the NaN pattern and the pixel counts, exactly
    assert np.array_equal(got["fit_status"], ref["fit_status"]) and np.array_equal(got["fit_npix"], ref["fit_npix"])
    for k in ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_chi2"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
    assert np.isfinite(got["fit_gram"]).all() and np.isfinite(got["fit_proj"]).all()    # no NaN of D or W reached a sum
    st = dict(zip(names, got["fit_status"]))
    assert (st["zero"] == 4).all() and (st["duplicate"] == 5).all()
    assert (got["fit_npix"][[i for i, n in enumerate(names) if n == "outside"]] == 0).all()
    # step 1
    worst = {}
    for k, a in (("fit_gram", "gram_abs"), ("fit_proj", "proj_abs")):
        err = np.abs(got[k] - ref[k])
        assert (err <= 1e-12 * ref[a]).all(), k
        worst[k] = float((err / np.where(ref[a] > 0, ref[a], 1.0)).max() / 1e-12)
    # steps 2 - 5 per field and band, on the restatement's G
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
    print(f"{cs}/{nb}/{F}: worst fraction of each bound - " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def _check_chi2(tag, stamps, places, fp, D, W, got):
    """the GPU's chi-square against the restatement on the GPU's own amplitudes and statuses"""
    worst = 0.0
    for m in range(len(fp) - 1):
        lo, hi = int(fp[m]), int(fp[m + 1])
        chi2, npix, yard = fw.chi2_field(stamps[lo:hi], np.asarray(places[lo:hi], np.int64), D[m], W[m], got["fit_scale"][lo:hi],
                                         got["fit_status"][lo:hi])
        assert np.array_equal(got["fit_npix"][lo:hi], npix), m
        assert np.array_equal(np.isnan(got["fit_chi2"][lo:hi]), np.isnan(chi2)), m
        assert np.array_equal(np.isnan(chi2), got["fit_status"][lo:hi] == 4)
        ok = ~np.isnan(chi2)
        err = np.abs(got["fit_chi2"][lo:hi][ok] - chi2[ok])
        assert (err <= 1e-12 * yard[ok]).all(), (m, float((err / yard[ok]).max()))
        if ok.any():
            worst = max(worst, float((err / np.where(yard[ok] > 0, yard[ok], 1.0)).max() / 1e-12))
    print(f"{tag}: worst fraction of the chi-square bound {worst:.1e}")


@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_chi_square_against_the_restatement_on_the_gpus_amplitudes(cs, nb, F):
    _, stamps, places, fp, D, W, _ = _wscene(cs, nb, F)
    got = _wgpu(cs, nb, F)
    _check_chi2(f"{cs}/{nb}/{F}", stamps, places, fp, D, W, got)
    ok = got["fit_status"] != 4
    assert (got["fit_chi2"][ok] >= 0).all() and (got["fit_npix"][ok] > 0).all()
    # the noise of the scene is 0.05 and W is not its inverse variance: chi2 / npix is of the order of 0.05^2 <W> where the fit
    # explains the pixels
    big = slice(int(fp[4]), int(fp[5]))
    ratio = got["fit_chi2"][big] / got["fit_npix"][big]
    assert (ratio < 10 * 0.05 ** 2 * 2.125).all()


def test_chi_square_with_more_neighbours_than_a_tile_and_more_galaxies_than_threads():
    """The field of 300 stamps of 9 px on a 3-px grid of tests/test_gpu_fit_flux.py, one band: a galaxy has up to 25 neighbours
    - and with a 1-px grid below, more than the 64 of one staging tile -, the rows of the adjacency and every 64- or
    256-strided loop take several turns."""
    cs, F, n = 9, 64, 300
    rng = np.random.default_rng(9)
    cells = np.arange(n)
    places = np.stack([(cells // 18) * 3, (cells % 18) * 3], axis=1).astype(np.int32)
    places[:4] = [[-4, -4], [F - 5, 2], [3, F - 4], [F - 6, F - 6]]
    stamps = np.stack([fo.elliptical_gaussian(cs, (1.4, rng.uniform(-0.3, 0.3), 1.4), rng.uniform(-0.5, 0.5, 2), rng.uniform(0.5, 2.0))
                       for _ in range(n)])[..., None].astype(np.float32)
    D = rng.normal(0.0, 0.05, size=(1, F, F, 1))
    for i in range(n):
        ra, rz, ca, cz = fo.clip(places[i], cs, F)
        D[0, ra:rz, ca:cz] += stamps[i, ra - places[i, 0]:rz - places[i, 0], ca - places[i, 1]:cz - places[i, 1]].astype(np.float64)
    wrng = np.random.default_rng(7100 + cs)
    W, D = _spoil(wrng, _draw_weights(wrng, D.shape, cs), D)
    got = _ctx().scene_fit_flux(stamps, places, D, weight_fields=W)
    assert (got["fit_status"] == 0).sum() > 290
    _check_chi2("300 x 9 px", stamps, places, [0, n], D, W, got)
    # 120 stamps one pixel apart in an 8 x 15 block: every one overlaps every other, degree 120 - the neighbour list goes
    # through the staging tile of 64 in two turns.  The fit drops what it cannot tell apart; the chi-square is compared on
    # whatever amplitudes and statuses it gives
    n2 = 120
    k = np.arange(n2)
    places2 = np.stack([20 + k // 15, 20 + k % 15], axis=1).astype(np.int32)
    got2 = _ctx().scene_fit_flux(stamps[:n2], places2, D, weight_fields=W, min_pivot=1e-3)
    assert np.isin(got2["fit_status"], (0, 5)).all() and (got2["fit_status"] == 0).any()
    _check_chi2("120 x 9 px, degree 120", stamps[:n2], places2, [0, n2], D, W, got2)


@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_a_mask_is_a_crop(cs, nb, F):
    _, stamps, places, fp, D = _scene(cs, nb, F)
    m, Fc = 4, F - cs // 2
    lo, hi = int(fp[m]), int(fp[m + 1])
    W = np.zeros((1, F, F, nb))
    W[:, :Fc, :Fc] = 1.0
    Dm = D[m:m + 1].copy()
    Dm[W == 0.0] = np.nan
    got = _ctx().scene_fit_flux(stamps[lo:hi], places[lo:hi], Dm, weight_fields=W)
    want = _ctx().scene_fit_flux(stamps[lo:hi], places[lo:hi], np.ascontiguousarray(D[m:m + 1, :Fc, :Fc]))
    assert np.array_equal(got["fit_status"], want["fit_status"]) and (got["fit_status"] == 0).sum() > nb * NBIG // 2
    for b in range(nb):
        ok = want["fit_status"][:, b] == 0
        err = np.abs(got["fit_scale"][ok, b] - want["fit_scale"][ok, b])
        assert (err <= 1e-10 * np.abs(want["fit_scale"][ok, b]).max()).all(), b
    assert np.array_equal(np.isnan(got["fit_scale"]), np.isnan(want["fit_scale"]))


@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_rows_keep_their_bits(cs, nb, F):
    _, stamps, places, fp, D, W, _ = _wscene(cs, nb, F)
    ctx = _ctx()
    got = _wgpu(cs, nb, F)
    again = ctx.scene_fit_flux(stamps, places, D, field_ptr=fp, weight_fields=W)
    for k in WKEYS:
        assert _eq(again[k], got[k]), k
    # the fields and the weights in reverse order
    order = np.concatenate([np.arange(fp[m], fp[m + 1]) for m in range(5, -1, -1)])
    fp_r = np.concatenate([[0], np.cumsum(np.diff(fp)[::-1])])
    moved = ctx.scene_fit_flux(stamps[order], places[order], D[::-1], field_ptr=fp_r, weight_fields=W[::-1])
    for k in WKEYS:
        assert _eq(moved[k], got[k][order]), k
    # one field alone in the call, its weights given as one field
    for m in (0, 3, 4):
        lo, hi = int(fp[m]), int(fp[m + 1])
        one = ctx.scene_fit_flux(stamps[lo:hi], places[lo:hi], D[m:m + 1], weight_fields=W[m])
        for k in WKEYS:
            assert _eq(one[k], got[k][lo:hi]), (m, k)
    # a scratch that holds the crowded field and no more: three sub-ranges, each with its own adjacency
    tight = nb * NBIG * NBIG * 8
    split = ctx.scene_fit_flux(stamps, places, D, field_ptr=fp, scratch_bytes=tight, weight_fields=W)
    for k in WKEYS:
        assert _eq(split[k], got[k]), k


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_host_call(dtype, monkeypatch):
    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(5, F2, seed=11)
    starts, places, fp = _windows(F2, COUNTS, seed=5)
    rng = np.random.default_rng(7100 + CS)
    W, _ = _spoil(rng, _draw_weights(rng, fields.shape, CS), fields)
    seed = 77
    stamps = eng.infer_fields_keep(fields, starts, fp, seed=seed)["loc"]
    want = ctx.scene_fit_flux(stamps, places, fields, field_ptr=fp, weight_fields=W)
    rows = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    print(f"[{dtype}] fit_status of the {len(starts)} network stamps x {NB} bands: "
          f"{np.bincount(want['fit_status'].ravel(), minlength=6).tolist()}")
    assert (want["fit_status"] == 0).any() and np.isfinite(want["fit_chi2"][want["fit_status"] == 0]).all()

    got = eng.infer_fields_measure_fit_weighted(fields, starts, fp, places, W, seed=seed)
    assert sorted(got) == sorted(tuple(rows) + WKEYS)
    for k in WKEYS:
        assert _eq(got[k], want[k]), k
    for k in rows:                                                # every shared output has infer_fields_measure's bits
        assert _eq(got[k], rows[k]), k
    # catalogue-only: no field is composited
    only = eng.infer_fields_measure_fit_weighted(fields, starts, fp, places, W, seed=seed, return_fields=False)
    assert sorted(only) == sorted(CAT + ("mse_center",) + WKEYS)
    for k in only:
        assert _eq(only[k], got[k]), k
    # grouped.  A field is fb = 131 * 131 * 6 * 8 = 823 728 bytes.  With the result fields a resident field takes five of them -
    # the source field, mean, stddev, residual and now the weight field: per_field = 5 fb = 4 118 640 bytes, so 13 MiB (13 631
    # 488 bytes) hold three and not four.  The catalogue-only form keeps the source and the weight field: per_field = 2 fb = 1
    # 647 456 bytes, 5 MiB (5 242 880) hold three and not four.  Three resident fields: the first group is fields 0 .. 2, and
    # field 2 (stamps 30 .. 179, chunks of 64) is carried into the second group, where its fit runs
    fb = F2 * F2 * NB * 8
    assert 3 * 5 * fb <= 13 << 20 < 4 * 5 * fb and 3 * 2 * fb <= 5 << 20 < 4 * 2 * fb
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "13")
    grouped = eng.infer_fields_measure_fit_weighted(fields, starts, fp, places, W, seed=seed)
    for k in got:
        assert _eq(grouped[k], got[k]), k
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "5")
    g2 = eng.infer_fields_measure_fit_weighted(fields, starts, fp, places, W, seed=seed, return_fields=False)
    for k in only:
        assert _eq(g2[k], only[k]), k
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    # the unweighted call beside it is what it was; M = 1 is the single-field view
    plain = eng.infer_fields_measure_fit(fields, starts, fp, places, seed=seed, return_fields=False)
    w0 = ctx.scene_fit_flux(stamps, places, fields, field_ptr=fp)
    assert all(_eq(plain[k], w0[k]) for k in KEYS) and "fit_chi2" not in plain
    m = 3
    s1, p1 = starts[fp[m]:fp[m + 1]], places[fp[m]:fp[m + 1]]
    one = eng.infer_cutouts_measure_fit_weighted(fields[m], s1, p1, W[m], seed=seed)
    st1 = eng.infer_fields_keep(fields[m:m + 1], s1, [0, len(s1)], seed=seed)["loc"]
    w1 = ctx.scene_fit_flux(st1, p1, fields[m:m + 1], weight_fields=W[m])
    assert "mean_field" in one and all(_eq(one[k], w1[k]) for k in WKEYS)


def test_deblend_field_batch_takes_the_weights():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    fields = _blob_fields(3, F2, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-45, 46, size=(n, 2)).astype(np.float64) for n in (20, 0, 45)]
    W = _draw_weights(np.random.default_rng(7100 + CS), fields.shape, CS)

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds
        return DeblendFieldBatch(net, fields, CS, NB)

    a, b, c, d = batch(), batch(), batch(), batch()
    res = a.deblend_fields(dists, on_device=True, measure=True, fit_flux=True, fit_weights=W)
    plain = b.deblend_fields(dists, on_device=True, measure=True)
    host = c.deblend_fields(dists, measure=True)                  # the default path: stamps and catalogue on the host
    names = tuple(n[0] for n in ms.fit_flux_weighted_dtype(NB))
    want_cols = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) +
                         DeblendFieldBatch.fit_flux_weighted_columns(NB))
    for m, (r, p, h) in enumerate(zip(res, plain, host)):
        assert r.dtype == want_cols and len(r) == len(p)
        for k in p.dtype.names:                                   # the columns of the call without it, value for value
            if k != "shifts":
                assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].base.kind == "f"), k
        if not len(r):
            continue
        mean = np.stack([np.asarray(x) for x in h["output_images_mean"]])
        places = int((F2 - CS) / 2) + dists[m].astype(np.int64)
        want = ms.fit_fluxes_weighted(mean, places, fields[m], W[m], catalogue=h, ctx=c._ctx)
        for k in names:
            assert np.array_equal(r[k], want[k], equal_nan=True), (m, k)
        ok = r["fit_status"] == 0
        assert ok.any() and np.isfinite(r["flux_fit"][ok]).all() and (r["fit_scale_err"][ok] > 0).all()
        assert np.isfinite(r["fit_chi2"][ok]).all() and (r["fit_npix"][ok] > 0).all()
    cat = d.deblend_fields(dists, on_device=True, measure=True, fit_flux=True, fit_weights=W, return_fields=False)
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
    W1 = _draw_weights(np.random.default_rng(7100 + CS), fields.shape, CS)
    good = eng.infer_fields_measure_fit_weighted(fields, starts, fp, places, W1, seed=3)

    n, nb = 5, NB
    ptr = lambda a: None if a is None else (_dp(a) if a.dtype == np.float64 else _fp(a) if a.dtype == np.float32 else _ip(a))   # noqa: E731
    cat = [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    seven = lambda n, nb: [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, nb), np.int32),   # noqa: E731
                           np.zeros((n, nb)), np.zeros((n, nb), np.int32)]
    ff = seven(n, nb)
    f2, N, args = Engine._field_args(fields, starts, fp, places)

    def pipeline(fpar=None, out=None, weights=W1, no_params=False, a=None):
        par = _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
        fpar = fpar or fit_flux_params()
        _lib.check(lib.dv_infer_fields_measure_fit_weighted(eng._h, *(args if a is None else a), 9, C.byref(par), None, None, None,
                                                            None, *map(ptr, cat), None if no_params else C.byref(fpar),
                                                            ptr(weights), *map(ptr, ff if out is None else out)))

    P, pl, D = np.ones((3, 31, 31, 3), np.float32), np.zeros((3, 2), np.int32), np.zeros((2, 40, 40, 3))
    Wd = np.ones_like(D)
    ff2 = seven(3, 3)

    def scene(stamps=P, places=pl, fptr=(0, 2, 3), n=3, data=D, weights=Wd, fpar=None, out=None, no_params=False):
        fpar = fpar or fit_flux_params()
        fptr = np.asarray(fptr, np.int64)
        _lib.check(lib.dv_scene_fit_flux_weighted(ctx._h, ptr(stamps), ptr(places), fptr.ctypes.data_as(C.POINTER(C.c_int64)), n, 31,
                                                  3, ptr(data), ptr(weights), len(fptr) - 1, 40,
                                                  None if no_params else C.byref(fpar), *map(ptr, ff2 if out is None else out)))

    for call in (pipeline, scene):
        with pytest.raises(DvError, match="params must be given"):
            call(no_params=True)
        with pytest.raises(DvError, match="weight_fields must be given"):
            call(weights=None)
        for fpar, msg in ((_lib.DvFitFluxParams(0.0, 1 << 20), "min_pivot"), (_lib.DvFitFluxParams(1e-8, 0), "scratch_bytes")):
            with pytest.raises(DvError, match=msg):
                call(fpar=fpar)
        for k in range(7):                                        # a missing output, the two new ones included
            out = list(ff if call is pipeline else ff2)
            out[k] = None
            with pytest.raises(DvError, match="must all be given"):
                call(out=out)
    # the scratch refusal and the field of 1025 stamps, in both calls
    with pytest.raises(DvError, match=rf"field 0 has 5 galaxies.*{NB * 25 * 8} bytes of scratch"):
        pipeline(fpar=_lib.DvFitFluxParams(1e-8, NB * 25 * 8 - 1))
    with pytest.raises(DvError, match="field 0 has 2 galaxies"):
        scene(fpar=_lib.DvFitFluxParams(1e-8, 3 * 4 * 8 - 1))
    many = 1025
    _, _, big_args = Engine._field_args(fields, np.zeros((many, 2), np.int32), [0, many], np.zeros((many, 2), np.int32))
    with pytest.raises(DvError, match="field 0 has 1025 galaxies, the dense fit takes at most 1024"):
        pipeline(a=big_args)
    chain = np.stack([np.zeros(many), (np.arange(many) % 3) * 30], axis=1).astype(np.int32)
    with pytest.raises(DvError, match="field 1 has 1025 galaxies, the dense fit takes at most 1024"):
        ctx.scene_fit_flux(np.ones((1 + many, 31, 31, 3), np.float32), np.concatenate([pl[:1], chain]), D, field_ptr=[0, 1, 1 + many],
                           weight_fields=Wd)
    # a wrong weight shape never reaches the library
    for bad in (W1[:, :-1], W1[..., :3], np.concatenate([W1, W1])):
        with pytest.raises(ValueError, match="expected weight fields of the shape of the data fields"):
            eng.infer_fields_measure_fit_weighted(fields, starts, fp, places, bad, seed=3)
        with pytest.raises(ValueError, match="expected weight fields of the shape of the data fields"):
            ctx.scene_fit_flux(np.ones((5, CS, CS, NB), np.float32), places, fields, weight_fields=bad)
    # the smallest scratch that takes the larger field runs: two identical stamps of ones at one place and a third in a field
    # of its own, on fields of zeros under unit weights - the later twin is dropped and keeps amplitude 1, which the first must
    # undo; the scene is reproduced exactly, so every chi-square is 0 on 961 pixels
    scene(fpar=_lib.DvFitFluxParams(1e-8, 3 * 4 * 8))
    assert ff2[4].tolist() == [[0] * 3, [5] * 3, [0] * 3] and (ff2[2] == 961.0).all() and (ff2[6] == 961).all()
    assert np.allclose(ff2[0], [[-1.0] * 3, [1.0] * 3, [0.0] * 3], rtol=0, atol=1e-12) and np.abs(ff2[5]).max() < 1e-20
    scene(n=0, fptr=(0, 0, 0), stamps=None, places=None, out=[None] * 7)
    # the engine completes a correct call afterwards, with the bits it gave before
    again = eng.infer_fields_measure_fit_weighted(fields, starts, fp, places, W1, seed=3)
    for k in good:
        assert _eq(again[k], good[k]), k
    pipeline()
    ref = eng.infer_fields_measure_fit_weighted(fields, starts, fp, places, W1, seed=9, return_fields=False)
    assert all(_eq(a, ref[k]) for a, k in zip(ff, WKEYS))
