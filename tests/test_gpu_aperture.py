"""The aperture photometry on the GPU (dv_scene_aperture, dv_infer_fields_measure_aper, DeblendFieldBatch(measure=True,
apertures=...)) against the numpy restatement of tests/aperture_oracle.py, and the pipeline stage
against the stamp-level call, bit for bit.  Both sides start from the same catalogue rows (the GPU's own measurement), so the
comparison is of the photometry alone.  The bounds are those of the specification: aper_status and aper_flags equal on every
row, every sum within 1e-12 of the sum of the absolute terms (the bound that holds for any summation order), and - the
restatement's tie margins are asserted to allow it on every row - the areas and the flux radii bit for bit: the areas are
sums of whole numbers, and with no decision flipped the bisection is exact halving from rho_auto.  A bisection converges on a
radius at which a sub-pixel crosses the boundary - F is a step function -, so its last tests come within rho_auto 2^-iters of
a tie by construction: the comparisons against the restatement halve 20 times, which leaves the sub-pixel margin above the
1e-9 the specification asks for (32 halvings end at 2e-10); the pipeline tests run the default 32.  The stamps avoid exact
ties too: no centroid on a pixel centre with a radius whose square is a multiple of 1 / 25."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import aperture_oracle as ao
from tests import measure_oracle as mo

pytestmark = pytest.mark.gpu

CAT = ("flux", "flux_err", "shape", "iters", "status")
AP = ("ap_flux", "ap_flux_err", "ap_area", "flux_auto", "flux_auto_err", "kron", "flux_rho", "aper_flags", "aper_status")
ARCH31 = dict(input_shape=(31, 31, 6), latent_dim=16, filters=[32, 64], kernels=[3, 3])
CS, NB = 31, 6
COUNTS = [30, 0, 150, 7, 40]      # one empty field, one with more stamps than max_batch = 64: chunks cross field boundaries
MARGIN_SUB, MARGIN_BIS = 1e-9, 1e-11
BISECT = 20                       # halvings in the comparisons against the restatement (see above)


def _ctx():
    from debvader_amd import engine as E

    return E.default_context()


def _planes(cs, full):
    """(name, plane (cs, cs)): the families of the specification"""
    rng = np.random.default_rng(700 + cs)
    ctr = (cs - 1) / 2.0
    rr, cc = np.arange(cs, dtype=np.float64)[:, None], np.arange(cs, dtype=np.float64)[None, :]
    fam = [(4.0, 0.0, 4.0), (6.0, 1.5, 3.0), (9.0, -2.0, 5.0), (2.25, 0.3, 1.8), (16.0, 3.0, 9.0)]
    out = [("iteration limit", mo.gaussian_stamp(cs, (7.0, 2.0, 5.0), (1.5, -0.8)) + 0.002)]      # measured with max_iter = 3
    for k in range(10 if full else 1):
        out.append(("gaussian", mo.gaussian_stamp(cs, fam[k % 5], rng.uniform(-0.5, 0.5, size=2), amp=rng.uniform(0.5, 3.0))))
    for k in range(11 if full else 1):                       # relu'd Gaussians with sigma = 0.02 noise
        a, b = rng.uniform(2.0, 9.0, size=2)
        M = (a, rng.uniform(-0.6, 0.6) * np.sqrt(a * b), b)
        g = mo.gaussian_stamp(cs, M, rng.uniform(-3.0, 3.0, size=2), amp=rng.uniform(0.5, 3.0))
        out.append(("noisy gaussian", np.maximum(g + rng.normal(0.0, 0.02, size=g.shape), 0.0)))
    for off in [(0.13, -0.21), (-0.7, 1.2), (2.4, -1.9), (0.3, 0.4)][:4 if full else 1]:    # wide: kron_factor r1 decides rho_auto
        out.append(("exponential", np.exp(-np.hypot(rr - ctr - off[0], cc - ctr - off[1]) / 2.5)))
    for k in range(4 if full else 1):                        # two overlapping blobs
        o1, o2 = rng.uniform(-2.0, 2.0, size=2), rng.uniform(-2.0, 2.0, size=2) + (3.0, 4.0)
        out.append(("two blobs", mo.gaussian_stamp(cs, (6.0, 0.0, 6.0), o1) + 0.6 * mo.gaussian_stamp(cs, (7.0, 1.0, 5.0), o2)))
    for k in range(3 if full else 1):                        # a blob towards a corner, as far as the iteration finds it from the
        # centre: 7 px from two edges of a 31-px stamp, whose wide apertures are truncated
        out.append(("corner", mo.gaussian_stamp(cs, (3.0, 0.4, 2.5), (-8.137 - 0.313 * k, 7.811 + 0.217 * k))))
    # no light within 13 px of the centre: with the row of the first Gaussian (sigma 2 px, _case) the kron_limit ellipse is empty
    hole = np.where(np.hypot(rr - ctr, cc - ctr) > 13.0, 0.4, 0.0)
    out += [("constant", np.full((cs, cs), 0.7)), ("zero", np.zeros((cs, cs))), ("no kron", hole)]
    return out


@functools.lru_cache(maxsize=None)
def _case(cs, nb, full, K, J, s, err):
    """(names, mean, stddev or None, the GPU's catalogue rows, the parameters, the oracle's rows): computed once, never
    written to"""
    planes = _planes(cs, full)
    band = 2
    rng = np.random.default_rng(13 * cs + nb)
    mean = np.zeros((len(planes), cs, cs, nb), np.float32)
    for i, (_, p) in enumerate(planes):
        for b in range(nb):
            mean[i, :, :, b] = p if b == band else rng.uniform(0.3, 2.0) * p + rng.uniform(-0.05, 0.1, size=p.shape)
    stddev = rng.uniform(0.01, 0.1, size=mean.shape).astype(np.float32) if err else None
    cat = _ctx().scene_measure(mean, band=band)
    limit = _ctx().scene_measure(mean[:1], band=band, max_iter=3)
    for k in ("shape", "iters", "status"):
        cat[k][0] = limit[k][0]
        cat[k][-1] = cat[k][1]                                    # the hole is measured with the first Gaussian's row
    par = ao.params(radii={0: (), 1: (5.3,), 3: (3.1, 5.3, 8.15), 8: (1.3, 2.45, 3.1, 4.15, 5.3, 6.45, 8.15, 11.3)}[K],
                    fractions=(0.2, 0.5, 0.8, 0.9)[:J], subsample=s, bisect_iters=BISECT)
    ref = ao.aperture(mean, stddev, cat["shape"], cat["status"], band, par, shortcut=True)
    for a in (mean,) + tuple(cat.values()) + (() if stddev is None else (stddev,)):
        a.flags.writeable = False
    return [n for n, _ in planes], mean, stddev, cat, par, ref


def _gpu(mean, stddev, cat, par, band=2, ctx=None):
    return (ctx or _ctx()).scene_aperture(mean, cat["shape"], cat["status"], stddev, radii=par["radii"], fractions=par["fractions"],
                                          band=band, subsample=par["subsample"], kron_factor=par["kron_factor"],
                                          kron_min=par["kron_min"], kron_limit=par["kron_limit"],
                                          bisect_iters=par["bisect_iters"])


def _compare(names, got, ref, par, err, what):
    K, J = len(par["radii"]), len(par["fractions"])
    band = 2
    worst = dict(ap=0.0, err=0.0, auto=0.0, auto_err=0.0, r1=0.0)
    close = lambda g, r, scale: float(np.max(np.abs(g - r) / scale, initial=0.0))     # noqa: E731
    for i, (name, w) in enumerate(zip(names, ref)):
        tag = (what, i, name)
        assert got["aper_status"][i] == w["status"] and got["aper_flags"][i] == w["flags"], tag
        if w["status"] == ao.INELIGIBLE:
            for k in AP[:7]:
                assert k not in got or np.isnan(got[k][i]).all(), tag + (k,)
            continue
        # no decision of this row is close enough to a tie for another summation order to flip it
        assert w["margin_sub"] > MARGIN_SUB and w["margin_bis"] > MARGIN_BIS, tag + (w["margin_sub"], w["margin_bis"])
        assert np.array_equal(got["ap_area"][i], w["ap_area"]), tag
        tiny = np.finfo(np.float64).tiny
        worst["ap"] = max(worst["ap"], close(got["ap_flux"][i], w["ap_flux"], w["ap_abs"] + tiny))
        if err:
            worst["err"] = max(worst["err"], close(got["ap_flux_err"][i] ** 2, w["ap_var"], w["ap_var"] + tiny))
        if w["status"] == ao.NO_KRON:
            for k in ("flux_auto", "flux_auto_err", "kron", "flux_rho"):
                assert k not in got or np.isnan(got[k][i]).all(), tag + (k,)
            continue
        r1, rho_auto, area = got["kron"][i]
        # r1 = A / B: an error of 1e-12 sum |a| in A and of 1e-12 sum |b| in B moves it by 1e-12 (sum |a| + r1 sum |b|) / B
        A_abs, B_abs = w["kron_abs"]
        worst["r1"] = max(worst["r1"], abs(r1 - w["kron"][0]) / ((A_abs + abs(w["kron"][0]) * B_abs) / abs(w["kron_sums"][1])))
        if w["flags"] & ao.FLAG_KRON_MIN:
            assert rho_auto == par["kron_min"], tag
        else:
            assert rho_auto == np.float64(par["kron_factor"]) * r1, tag
        assert area == w["kron"][2], tag
        worst["auto"] = max(worst["auto"], close(got["flux_auto"][i], w["flux_auto"], w["auto_abs"] + tiny))
        if err:
            worst["auto_err"] = max(worst["auto_err"], close(got["flux_auto_err"][i] ** 2, w["auto_var"], w["auto_var"] + tiny))
        for j in range(J):
            assert got["flux_rho"][i, j] == ao.replay(rho_auto, w["decisions"][j]), tag + (j,)
            if rho_auto == w["kron"][1]:
                assert got["flux_rho"][i, j] == w["flux_rho"][j], tag + (j,)
    st = np.array([w["status"] for w in ref])
    print(f"{what}: aper_status {np.bincount(st, minlength=8).tolist()}, kron_min decides {sum(bool(w['flags'] & ao.FLAG_KRON_MIN) for w in ref)} "
          f"rows, truncated {sum(bool(w['flags'] & 0x3ff) for w in ref)}; sums relative to the absolute sums: " +
          ", ".join(f"{k} {v:.1e}" for k, v in worst.items()) +
          f"; tie margins >= {min(w['margin_sub'] for w in ref):.1e} (sub-pixels), {min(w['margin_bis'] for w in ref):.1e} (bisection)")
    assert max(worst.values()) <= 1e-12, worst


@pytest.mark.parametrize("cs,nb,full,K,J,s,err", [(31, 3, True, 8, 4, 5, True), (31, 6, True, 1, 0, 1, False),
                                                  (31, 6, True, 3, 3, 5, True), (59, 6, False, 0, 4, 5, True),
                                                  (59, 6, False, 3, 3, 5, False)])
def test_scene_aperture_against_the_oracle(cs, nb, full, K, J, s, err):
    names, mean, stddev, cat, par, ref = _case(cs, nb, full, K, J, s, err)
    assert len(names) == (36 if full else 9)
    # the restatement alone first: the families end where the specification says
    st = dict(zip(names, (w["status"] for w in ref)))
    assert cat["status"][0] == 2 and st["iteration limit"] == ao.OK and st["zero"] == ao.INELIGIBLE and st["no kron"] == ao.NO_KRON
    assert st["gaussian"] == st["noisy gaussian"] == st["exponential"] == st["two blobs"] == st["corner"] == ao.OK
    flags = {n: w["flags"] for n, w in zip(names, ref)}
    assert flags["gaussian"] & ao.FLAG_KRON_MIN and not flags["exponential"] & ao.FLAG_KRON_MIN
    if cs == 31:
        assert flags["corner"] & ao.FLAG_LIMIT and (K < 3 or flags["corner"] & (1 << (K - 1)))
    got = _gpu(mean, stddev, cat, par)
    assert sorted(got) == sorted(k for k in AP if err or not k.endswith("_err"))
    assert got["ap_flux"].shape == (len(names), K, nb) and got["flux_rho"].shape == (len(names), J)
    _compare(names, got, ref, par, err, f"gpu vs oracle {cs}/{nb}/K{K}/J{J}/s{s}")


def test_largest_stamp_fits_the_lds():
    """One stamp of 90 px: 8 * 90^2 + 384 bytes of dynamic LDS, the largest layout dv_infer_fields_measure accepts"""
    cs = 90
    p = mo.gaussian_stamp(cs, (30.0, 8.0, 22.0), (3.37, -2.61)) + 0.5 * mo.gaussian_stamp(cs, (5.0, 0.0, 5.0), (-20.0, 25.0))
    mean = np.stack([p, 0.5 * p, p], axis=-1)[None].astype(np.float32)
    stddev = np.full(mean.shape, 0.05, np.float32)
    cat = _ctx().scene_measure(mean, band=2)
    par = ao.params(radii=(3.1, 5.3, 8.15), bisect_iters=BISECT)
    ref = ao.aperture(mean, stddev, cat["shape"], cat["status"], 2, par, shortcut=True)
    assert cat["status"][0] == 0 and ref[0]["status"] == ao.OK
    _compare(["gaussian"], _gpu(mean, stddev, cat, par), ref, par, True, "gpu vs oracle 90/3")


def test_a_row_has_the_same_bits_wherever_it_sits():
    names, mean, stddev, cat, par, ref = _case(31, 6, True, 3, 3, 5, True)
    got = _gpu(mean, stddev, cat, par)
    perm = np.random.default_rng(1).permutation(len(names))
    shuffled = _gpu(mean[perm], stddev[perm], {k: v[perm] for k, v in cat.items()}, par)
    for k in AP:
        assert np.array_equal(shuffled[k], got[k][perm], equal_nan=True), k
    for i in (1, 14, 30):                                         # one galaxy alone
        alone = _gpu(mean[i:i + 1], stddev[i:i + 1], {k: v[i:i + 1] for k, v in cat.items()}, par)
        for k in AP:
            assert np.array_equal(alone[k][0], got[k][i], equal_nan=True), (i, k)
    other = np.array(mean)                                       # the other bands' contents changed
    other[..., :2] = 0.5
    other[..., 3:] *= 1.7
    o = _gpu(other, stddev, cat, par)
    for k in ("ap_area", "kron", "flux_rho", "aper_flags", "aper_status"):
        assert np.array_equal(o[k], got[k], equal_nan=True), k
    for k in ("ap_flux", "ap_flux_err", "flux_auto", "flux_auto_err"):
        assert np.array_equal(o[k][..., 2], got[k][..., 2], equal_nan=True), k
    assert not np.array_equal(o["flux_auto"][..., 0], got["flux_auto"][..., 0], equal_nan=True)
    # without the stddev stamp the fluxes keep their bits
    bare = _gpu(mean, None, cat, par)
    assert "ap_flux_err" not in bare and all(np.array_equal(bare[k], got[k], equal_nan=True) for k in bare)


# ---- the pipeline stage -------------------------------------------------------------------------------------------------------

def _net(dtype, max_batch=64, seed=3):
    from debvader_amd.model import model

    net, _, _, _ = model.create_model_vae(**ARCH31, max_batch=max_batch, seed=seed, dtype=dtype)
    return net


def _blob_fields(M, F, seed, nblob=14):
    rng = np.random.default_rng(seed)
    out = rng.normal(0, 0.05, size=(M, F, F, NB))
    yy, xx = np.mgrid[:F, :F]
    for m in range(M):
        for _ in range(nblob):
            r, c = rng.uniform(15, F - 15, size=2)
            sig, a = rng.uniform(1.5, 3.0), rng.uniform(2.0, 9.0)
            out[m] += (a * np.exp(-0.5 * ((yy - r) ** 2 + (xx - c) ** 2) / sig ** 2))[:, :, None] * rng.uniform(0.5, 1.0, size=NB)
    return out


def _windows(F, counts, seed, hang=True):
    rng = np.random.default_rng(seed)
    n = int(np.sum(counts))
    starts = rng.integers(0, F - CS + 1, size=(n, 2)).astype(np.int32)
    places = starts.copy()
    if hang:
        k = rng.random(n) < 0.3
        places[k] = rng.integers(-CS + 3, F - 3, size=(int(k.sum()), 2))
    return starts, places, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_stamp_level_call(dtype, monkeypatch):
    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    F = 131
    fields = _blob_fields(5, F, seed=11)
    starts, places, fp = _windows(F, COUNTS, seed=5)
    seed = 77
    kw = dict(radii=(2.0, 4.5), fractions=(0.3, 0.5, 0.9))
    stamps = eng.infer_fields(fields, starts, fp, seed=seed)
    plain = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    want = ctx.scene_aperture(stamps["loc"], plain["shape"], plain["status"], stamps["scale"], **kw)
    print(f"[{dtype}] aper_status of the {len(starts)} network stamps: {np.bincount(want['aper_status'], minlength=8).tolist()}, "
          f"catalogue status {np.bincount(plain['status'], minlength=4).tolist()}")

    got = eng.infer_fields_measure_aper(fields, starts, fp, places=places, seed=seed, **kw)
    assert sorted(got) == sorted(tuple(plain) + AP)
    for k in plain:                                               # every shared output has infer_fields_measure's bits
        assert np.array_equal(got[k], plain[k]), k
    for k in AP:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), k
    # the catalogue-only call
    only = eng.infer_fields_measure_aper(fields, starts, fp, seed=seed, return_fields=False, **kw)
    assert sorted(only) == sorted(CAT + ("mse_center",) + AP)
    for k in only:
        assert np.array_equal(only[k], got[k], equal_nan=True), k
    # the fields uploaded in groups (see tests/test_gpu_fields_batch.py), with and without result fields
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "10")
    grouped = eng.infer_fields_measure_aper(fields, starts, fp, places=places, seed=seed, **kw)
    for k in got:
        assert np.array_equal(grouped[k], got[k], equal_nan=True), k
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "3")
    g2 = eng.infer_fields_measure_aper(fields, starts, fp, seed=seed, return_fields=False, **kw)
    for k in only:
        assert np.array_equal(g2[k], only[k], equal_nan=True), k
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    # other parameters reach the kernel, no radii and no fractions; M = 1 is the single-field view
    b0 = eng.infer_fields_measure_aper(fields, starts, fp, seed=seed, return_fields=False, band=0, max_iter=9, radii=(),
                                       fractions=(), subsample=3, kron_factor=2.0, kron_min=2.5, kron_limit=5.0)
    c0 = ctx.scene_measure(stamps["loc"], stamps["scale"], band=0, max_iter=9)
    w0 = ctx.scene_aperture(stamps["loc"], c0["shape"], c0["status"], stamps["scale"], band=0, radii=(), fractions=(), subsample=3,
                            kron_factor=2.0, kron_min=2.5, kron_limit=5.0)
    assert all(np.array_equal(b0[k], w0[k], equal_nan=True) for k in AP) and b0["ap_flux"].shape == (len(starts), 0, NB)
    assert np.array_equal(b0["shape"], c0["shape"]) and not np.array_equal(b0["kron"], want["kron"], equal_nan=True)
    s1, p1, fp1 = _windows(F, [70], seed=9)
    one = eng.infer_fields_measure_aper(fields[2:3], s1, fp1, places=p1, seed=seed, **kw)
    ref = eng.infer_cutouts_measure_aper(fields[2], s1, places=p1, seed=seed, **kw)
    assert "mean_field" in ref and np.array_equal(one["mean_fields"][0], ref["mean_field"])
    for k in CAT + AP:
        assert np.array_equal(one[k], ref[k], equal_nan=True), k


def test_deblend_field_batch_takes_apertures_on_the_device():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    F = 131
    fields = _blob_fields(3, F, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-30, 31, size=(n, 2)).astype(np.float64) for n in (20, 0, 45)]

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds (random per net)
        return net, DeblendFieldBatch(net, fields, CS, NB)

    plain = batch()[1].deblend_fields(dists, on_device=True, measure=True)
    net, d = batch()
    default = d.deblend_fields(dists, measure=True)              # the default path: the stamps come back to the host
    for apertures, fractions in (((3.0, 5.0, 8.0), None), ((), (0.5,))):
        kw = {} if fractions is None else {"flux_fractions": fractions}
        K, J = len(apertures), 3 if fractions is None else len(fractions)
        want_cols = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) +
                             DeblendFieldBatch.aperture_columns(NB, K, J))
        res = batch()[1].deblend_fields(dists, on_device=True, measure=True, apertures=apertures, **kw)
        only = batch()[1].deblend_fields(dists, on_device=True, measure=True, apertures=apertures, return_fields=False, **kw)
        for r, p, q, h in zip(res, plain, only, default):
            assert r.dtype == want_cols and len(r) == len(p)
            for k in p.dtype.names:                               # the columns of the same call without apertures
                if k != "shifts":
                    assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].base.kind == "f"), k
            for k in r.dtype.names:                               # return_fields=False: the same catalogue
                if k != "shifts":
                    assert np.array_equal(r[k], q[k], equal_nan=r.dtype[k].base.kind == "f"), k
            if len(r):
                mean = np.stack(list(h["output_images_mean"]))
                stddev = np.stack(list(h["output_images_stddev"]))
                cat = ms.measure_apertures(mean, stddev, radii=apertures, fractions=(0.2, 0.5, 0.8) if fractions is None else fractions,
                                           ctx=net._core.ctx)
                for k in cat.dtype.names:
                    assert np.array_equal(r[k], cat[k], equal_nan=cat.dtype[k].base.kind == "f"), k
        assert np.isfinite(np.concatenate([r["flux_auto"] for r in res])).any()


def test_refusals_come_before_any_gpu_work_and_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import Engine, _dp, _fp, _ip, aperture_params

    DvError, lib = _lib.DvError, _lib.lib
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    F = 131
    fields = _blob_fields(1, F, seed=11)
    starts, places, fp = _windows(F, [5], seed=5, hang=False)
    good = eng.infer_fields_measure_aper(fields, starts, fp, places=places, seed=3)

    n, nb, K, J = 5, NB, 3, 3
    cat = [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    rows = lambda n, nb: [np.zeros((n, K, nb)), np.zeros((n, K, nb)), np.zeros((n, K)), np.zeros((n, nb)), np.zeros((n, nb)),   # noqa: E731
                          np.zeros((n, 3)), np.zeros((n, J)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    ap = rows(n, nb)
    ptr = lambda a: None if a is None else (_dp(a) if a.dtype == np.float64 else _ip(a))     # noqa: E731
    f2, N, args = Engine._field_args(fields, starts, fp, places)
    mean_f, std_f, res_f = np.empty(f2.shape), np.empty(f2.shape), np.empty(f2.shape)

    def pipeline(par=None, apar=None, out=None, fields_out=(None, None, None), no_params=False):
        par = par or _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
        apar = apar or aperture_params()
        out = ap if out is None else out
        _lib.check(lib.dv_infer_fields_measure_aper(eng._h, *args, 9, C.byref(par), *fields_out, None, *map(ptr, cat),
                                                    None if no_params else C.byref(apar), *map(ptr, out)))

    st = np.zeros((2, 31, 31, 3), np.float32)
    sd = np.full((2, 31, 31, 3), 0.1, np.float32)
    sh, stat = np.zeros((2, 5)), np.zeros(2, np.int32)
    ap2 = rows(2, 3)

    def scene(x=st, s=sd, band=2, apar=None, out=None, shape=sh, no_params=False):
        apar = apar or aperture_params()
        out = ap2 if out is None else out
        _lib.check(lib.dv_scene_aperture(ctx._h, _fp(x), None if s is None else _fp(s), ptr(shape), _ip(stat), x.shape[0],
                                         x.shape[1], x.shape[3], band, None if no_params else C.byref(apar), *map(ptr, out)))

    def edited(**kw):
        p = aperture_params()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, v[0])[v[1]] = v[2]
            else:
                setattr(p, k, v)
        return p

    nan, inf = float("nan"), float("inf")
    for call in (pipeline, scene):
        with pytest.raises(DvError, match="params must be given"):
            call(no_params=True)
        for apar, msg in ((edited(n_radii=9), "0 .. 8 radii"), (edited(n_radii=-1), "0 .. 8 radii"),
                          (edited(n_fractions=5), "0 .. 4 fractions"), (edited(n_fractions=-1), "0 .. 4 fractions"),
                          (edited(r=("radii", 1, 0.0)), "radius 1"), (edited(r=("radii", 2, nan)), "radius 2"),
                          (edited(r=("radii", 0, inf)), "radius 0"), (edited(r=("radii", 0, -3.0)), "radius 0"),
                          (edited(f=("fractions", 0, 0.0)), "fraction 0"), (edited(f=("fractions", 2, 1.0)), "fraction 2"),
                          (edited(f=("fractions", 1, nan)), "fraction 1"),
                          (edited(subsample=0), "subsample"), (edited(subsample=10), "subsample"),
                          (edited(bisect_iters=0), "bisect_iters"), (edited(bisect_iters=61), "bisect_iters"),
                          (edited(kron_factor=0.0), "kron_factor"), (edited(kron_factor=nan), "kron_factor"),
                          (edited(kron_min=-1.0), "kron_min"), (edited(kron_min=inf), "kron_min"),
                          (edited(kron_limit=0.0), "kron_limit"), (edited(kron_limit=nan), "kron_limit")):
            with pytest.raises(DvError, match=msg):
                call(apar=apar)
        for k in range(9):
            out = list(ap if call is pipeline else ap2)
            out[k] = None
            with pytest.raises(DvError, match="must all be given|go together"):
                call(out=out)
    # a radius or a fraction beyond the count is not read; without radii or fractions their outputs may be null
    scene(apar=edited(n_radii=2, r=("radii", 2, nan)))
    none = list(ap2)
    none[0] = none[1] = none[2] = none[6] = None
    scene(apar=edited(n_radii=0, n_fractions=0), out=none)
    # stddev and the two errors go together
    with pytest.raises(DvError, match="go together"):
        scene(s=None)
    bare = list(ap2)
    bare[1] = bare[4] = None
    scene(s=None, out=bare)
    # everything dv_infer_fields_measure refuses
    for par, msg in ((_lib.DvMeasureParams(NB, 3.0, 1e-10, 200), "band"), (_lib.DvMeasureParams(2, 0.0, 1e-10, 200), "sigma0"),
                     (_lib.DvMeasureParams(2, 3.0, 0.0, 200), "tol"), (_lib.DvMeasureParams(2, 3.0, 1e-10, -1), "max_iter")):
        with pytest.raises(DvError, match=msg):
            pipeline(par=par)
    with pytest.raises(DvError, match="go together"):
        pipeline(fields_out=(_dp(mean_f), None, None))
    for kw, msg in ((dict(band=3), "band"), (dict(shape=None), "must all be given"),
                    (dict(x=np.zeros((1, 91, 91, 1), np.float32), s=np.zeros((1, 91, 91, 1), np.float32), band=0), "at most 90 pixels")):
        with pytest.raises(DvError, match=msg):
            scene(**kw)
    # the engine completes a correct call afterwards, with the bits it gave before
    again = eng.infer_fields_measure_aper(fields, starts, fp, places=places, seed=3)
    for k in good:
        assert np.array_equal(again[k], good[k], equal_nan=True), k
    pipeline(fields_out=(_dp(mean_f), _dp(std_f), _dp(res_f)))
    assert np.array_equal(mean_f, eng.infer_fields_composite(fields, starts, places, fp, seed=9)["mean_fields"])
    assert np.array_equal(ap[5], eng.infer_fields_measure_aper(fields, starts, fp, places=places, seed=9)["kron"], equal_nan=True)
