"""The adaptive moments on the observed field with the neighbours subtracted on the GPU (dv_scene_moments_fields,
dv_infer_fields_measure_moments_data, DeblendFieldBatch(moments_data=True)).

Bits that must hold: with D bit-identical to T every output is dv_scene_measure's; a row keeps its bits wherever it sits in a
batch; the pipeline stage has the bits of the host call, on both engines, with and without result fields and weights, with a
field carried across two groups of resident fields; a masked pixel reaches nothing.

Against the numpy restatement of tests/moments_fields_oracle.py, on noisy data: status and npix equal, iters equal or one
apart, flux_data within 1e-12 of the sum of |C| (at most 59^2 = 3481 terms of both signs times 2^-53 is 4e-13 for any order of
summation), and for the rows converged in both the centroid within 1e-8 px and M within 1e-8 (Mrr + Mcc) - the bounds of
tests/test_gpu_measure.py.  Their derivation holds under a condition: two iterations that stop below tol = 1e-10 with
contraction rho lie within 2 rho / (1 - rho) 1e-10 of each other.  rho is taken from the restatement's history, the largest
ratio of successive entries over the last five iterations, and only rows with rho <= 0.9 are compared (1.8e-9, a fifth of the
bound); at most 10 % of the converged rows may be left out.  The worst fraction of each bound is printed."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import measure_oracle as mo
from tests import moments_fields_oracle as mf
from tests.test_gpu_aperture import CAT, COUNTS, CS, NB, _blob_fields, _net, _windows
from tests.test_gpu_fit_flux import SHAPES, _scene

pytestmark = pytest.mark.gpu

KEYS = ("flux_data", "npix_data", "shape_data", "iters_data", "status_data")
F2 = 131


def _ctx():
    from debvader_amd import engine as E

    return E.default_context()


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _composite(stamps, places, fp, F):
    """T: the float64 sum of the float32 stamps of every field, in object order, the parts outside the field dropped"""
    n, cs, _, nb = stamps.shape
    T = np.zeros((len(fp) - 1, F, F, nb))
    for m in range(len(fp) - 1):
        for i in range(int(fp[m]), int(fp[m + 1])):
            pr, pc = int(places[i][0]), int(places[i][1])
            ra, rz, ca, cz = max(pr, 0), min(pr + cs, F), max(pc, 0), min(pc + cs, F)
            if rz > ra and cz > ca:
                T[m, ra:rz, ca:cz] += stamps[i, ra - pr:rz - pr, ca - pc:cz - pc].astype(np.float64)
    return T


def _clipped(places, cs, F):
    p = np.asarray(places, dtype=np.int64)
    rows = np.clip(np.minimum(p[:, 0] + cs, F) - np.maximum(p[:, 0], 0), 0, None)
    cols = np.clip(np.minimum(p[:, 1] + cs, F) - np.maximum(p[:, 1], 0), 0, None)
    return (rows * cols).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _host_scene(cs, nb, F):
    """The 71 galaxies in six fields of tests/test_gpu_fit_flux.py - alone, pairs, a triple, stamps over edges and corners, two
    wholly outside, an all-zero stamp, a duplicate, a crowded field, a field without stamps - with T the composite of the
    stamps and D that scene's data: the stamps at amplitudes 0.7 .. 1.3 plus noise 0.05.  Never written to."""
    names, stamps, places, fp, D = _scene(cs, nb, F)
    T = _composite(stamps, places, fp, F)
    T.flags.writeable = False
    return names, stamps, places, fp, T, D


@functools.lru_cache(maxsize=None)
def _host_gpu(cs, nb, F):
    _, stamps, places, fp, T, D = _host_scene(cs, nb, F)
    out = _ctx().scene_moments_fields(stamps, places, T, D, field_ptr=fp)
    for a in out.values():
        a.flags.writeable = False
    return out


def _against_the_restatement(tag, got, stamps, places, fp, T, D, W=None, cap=0.10, **par):
    """the comparison of the module docstring; returns the worst fraction of each bound"""
    hist = []
    ref = mf.moments_fields(stamps, places, fp, T, D, W, histories=hist, **par)
    assert np.array_equal(got["status_data"], ref["status_data"]), tag
    assert np.array_equal(got["npix_data"], ref["npix_data"]) and got["npix_data"].dtype == np.int32, tag
    assert (np.abs(got["iters_data"].astype(np.int64) - ref["iters_data"]) <= 1).all(), tag
    fin = np.isfinite(ref["flux_abs"])
    assert np.array_equal(np.isfinite(got["flux_data"]), np.isfinite(ref["flux_data"])), tag
    err = np.abs(got["flux_data"][fin] - ref["flux_data"][fin])
    assert (err <= 1e-12 * ref["flux_abs"][fin]).all(), tag
    worst = {"flux": float((err / np.where(ref["flux_abs"][fin] > 0, ref["flux_abs"][fin], 1.0)).max() / 1e-12) if fin.any() else 0.0}
    conv = np.nonzero(ref["status_data"] == 0)[0]
    rho = np.array([mf.late_contraction(hist[i]) for i in conv])
    keep = conv[rho <= 0.9]
    print(f"{tag}: status {np.bincount(ref['status_data'], minlength=4).tolist()}, {len(conv)} converged, {len(conv) - len(keep)} "
          f"left out (late rho > 0.9), worst kept rho {rho[rho <= 0.9].max() if len(keep) else 0.0:.3f}, iterations up to "
          f"{int(ref['iters_data'][conv].max()) if len(conv) else 0}, {int((got['iters_data'] != ref['iters_data']).sum())} rows one apart")
    assert len(conv) - len(keep) <= cap * len(conv), tag
    g, r = got["shape_data"][keep], ref["shape_data"][keep]
    cen = np.abs(g[:, :2] - r[:, :2]).max(axis=1) if len(keep) else np.zeros(0)
    mom = (np.abs(g[:, 2:] - r[:, 2:]).max(axis=1) / (r[:, 2] + r[:, 4])) if len(keep) else np.zeros(0)
    worst.update(centroid=float(cen.max() / 1e-8) if len(keep) else 0.0, M=float(mom.max() / 1e-8) if len(keep) else 0.0)
    print(f"{tag}: worst fraction of each bound - " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert (cen <= 1e-8).all() and (mom <= 1e-8).all(), tag
    return worst


# ---- 1: D bit-identical to T -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _network_scene(dtype, seed=77):
    """Five 131-pixel blob fields, 227 windows of the 31-pixel network; the first nine placements hang over each edge and each
    corner and one lies wholly outside.  (net, fields, starts, places, fp, mean stamps, mean fields)"""
    net = _net(dtype)
    eng = net._core.engine
    fields = _blob_fields(5, F2, seed=11)
    starts, places, fp = _windows(F2, COUNTS, seed=5)
    places[:9] = [[-10, 50], [F2 - 20, 50], [50, -12], [50, F2 - 9], [-5, -7], [-8, F2 - 11], [F2 - 6, -20], [F2 - 15, F2 - 4],
                  [-CS - 5, 10]]
    stamps = eng.infer_fields_keep(fields, starts, fp, seed=seed)["loc"]
    T = eng.infer_fields_composite(fields, starts, places, fp, seed=seed)["mean_fields"]
    for a in (fields, starts, places, fp, stamps, T):
        a.flags.writeable = False
    return net, fields, starts, places, fp, stamps, T


def test_data_with_the_bits_of_the_model_gives_the_bits_of_scene_measure():
    net, fields, starts, places, fp, stamps, T = _network_scene("float32")
    ctx = net._core.ctx
    want = ctx.scene_measure(stamps, None, band=2)
    got = ctx.scene_moments_fields(stamps, places, T, T.copy(), field_ptr=fp)
    assert sorted(got) == sorted(KEYS)
    for a, b in (("shape_data", "shape"), ("iters_data", "iters"), ("status_data", "status"), ("flux_data", "flux")):
        assert _eq(got[a], want[b]), a                                # every row
    npix = _clipped(places, CS, F2)
    assert npix[8] == 0 and (npix[:8] > 0).all() and (npix[:8] < CS * CS).all() and (npix == CS * CS).any()
    assert np.array_equal(got["npix_data"], np.repeat(npix[:, None], NB, axis=1)) and got["npix_data"].dtype == np.int32
    # the host scene too, and another band and other parameters reach the kernel
    for cs, nb, F in SHAPES:
        _, st, pl, fq, T2, _ = _host_scene(cs, nb, F)
        for par in (dict(band=2), dict(band=0, sigma0=2.0, tol=1e-8, max_iter=7)):
            w2 = _ctx().scene_measure(st, None, **par)
            g2 = _ctx().scene_moments_fields(st, pl, T2, T2, field_ptr=fq, **par)
            for a, b in (("shape_data", "shape"), ("iters_data", "iters"), ("status_data", "status"), ("flux_data", "flux")):
                assert _eq(g2[a], w2[b]), (cs, par, a)
            assert np.array_equal(g2["npix_data"][:, 0], _clipped(pl, cs, F))
        assert (g2["status_data"] == 2).any()                         # (max_iter = 7 ends some rows at the limit)


# ---- 2: batch independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_rows_keep_their_bits(cs, nb, F):
    _, stamps, places, fp, T, D = _host_scene(cs, nb, F)
    ctx = _ctx()
    got = _host_gpu(cs, nb, F)
    assert not _eq(got["shape_data"], ctx.scene_measure(stamps, None)["shape"])      # (the data are not the model)
    again = ctx.scene_moments_fields(stamps, places, T, D, field_ptr=fp)
    for k in KEYS:
        assert _eq(again[k], got[k]), k
    # the fields in reverse order
    order = np.concatenate([np.arange(fp[m], fp[m + 1]) for m in range(5, -1, -1)])
    fp_r = np.concatenate([[0], np.cumsum(np.diff(fp)[::-1])])
    moved = ctx.scene_moments_fields(stamps[order], places[order], T[::-1], D[::-1], field_ptr=fp_r)
    for k in KEYS:
        assert _eq(moved[k], got[k][order]), k
    # one field alone in the call
    for m in (0, 3, 4):
        lo, hi = int(fp[m]), int(fp[m + 1])
        one = ctx.scene_moments_fields(stamps[lo:hi], places[lo:hi], T[m:m + 1], D[m:m + 1])
        for k in KEYS:
            assert _eq(one[k], got[k][lo:hi]), (m, k)
    # the rows of another field permuted (T and D are inputs: they stay)
    perm = np.arange(len(stamps))
    lo, hi = int(fp[4]), int(fp[5])
    perm[lo:hi] = lo + np.random.default_rng(1).permutation(hi - lo)
    mixed = ctx.scene_moments_fields(stamps[perm], places[perm], T, D, field_ptr=fp)
    for k in KEYS:
        assert _eq(mixed[k], got[k][perm]), k


# ---- 3: the pipeline against the host call, both engines ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_host_call(dtype, monkeypatch):
    from tests.test_gpu_fit_flux_weighted import _draw_weights, _spoil

    net, fields, starts, places, fp, stamps, T = _network_scene(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    seed = 77
    rng = np.random.default_rng(7100 + CS)
    W, _ = _spoil(rng, _draw_weights(rng, fields.shape, CS), fields)       # (NaN in the data under some masked pixels)
    rows = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    fb = F2 * F2 * NB * 8
    # DV_FIELDS_GROUP_MB: the values of tests/test_gpu_fit_flux_groups.py.  With the result fields a resident field is the source
    # field and three result fields (and the weights): 10 (13) MiB hold three, so field 2 (stamps 30 .. 179, chunks of 64) is
    # carried from the first group into the second and its moments are taken there.  The catalogue-only form keeps the source field
    # and the device-side mean field (and the weights): 5 (10) MiB hold three (four) fields, and field 2 is carried again
    for weights, mb_fields, mb_only in ((None, "10", "5"), (W, "13", "10")):
        want = ctx.scene_moments_fields(stamps, places, T, fields, weight_fields=weights, field_ptr=fp)
        print(f"[{dtype}, weights {weights is not None}] status_data of the {len(starts)} network stamps: "
              f"{np.bincount(want['status_data'], minlength=4).tolist()}")
        got = eng.infer_fields_measure_moments_data(fields, starts, fp, places, weight_fields=weights, seed=seed)
        assert sorted(got) == sorted(tuple(rows) + KEYS)
        for k in KEYS:
            assert _eq(got[k], want[k]), k
        for k in rows:                                                # every shared output has infer_fields_measure's bits
            assert _eq(got[k], rows[k]), k
        only = eng.infer_fields_measure_moments_data(fields, starts, fp, places, weight_fields=weights, seed=seed, return_fields=False)
        assert sorted(only) == sorted(CAT + ("mse_center",) + KEYS)
        for k in only:
            assert _eq(only[k], got[k]), k
        per = (5 if weights is not None else 4) * fb
        assert 3 * per <= int(mb_fields) << 20 < 4 * per
        monkeypatch.setenv("DV_FIELDS_GROUP_MB", mb_fields)
        carried = eng.infer_fields_measure_moments_data(fields, starts, fp, places, weight_fields=weights, seed=seed)
        for k in got:
            assert _eq(carried[k], got[k]), k
        per = (3 if weights is not None else 2) * fb
        assert 3 <= (int(mb_only) << 20) // per <= 4
        monkeypatch.setenv("DV_FIELDS_GROUP_MB", mb_only)
        g2 = eng.infer_fields_measure_moments_data(fields, starts, fp, places, weight_fields=weights, seed=seed, return_fields=False)
        for k in only:
            assert _eq(g2[k], only[k]), k
        monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    assert not _eq(want["npix_data"], np.repeat(_clipped(places, CS, F2)[:, None], NB, axis=1))   # (the mask reached the kernel)
    # other parameters reach the kernel; M = 1 is the single-field view
    other = eng.infer_fields_measure_moments_data(fields, starts, fp, places, seed=seed, return_fields=False, band=0, sigma0=2.5, max_iter=9)
    w2 = ctx.scene_moments_fields(stamps, places, T, fields, field_ptr=fp, band=0, sigma0=2.5, max_iter=9)
    assert all(_eq(other[k], w2[k]) for k in KEYS) and not _eq(other["shape_data"], only["shape_data"])
    m = 3
    s1, p1 = starts[fp[m]:fp[m + 1]], places[fp[m]:fp[m + 1]]
    one = eng.infer_cutouts_measure_moments_data(fields[m], s1, p1, seed=seed)
    st1 = eng.infer_fields_keep(fields[m:m + 1], s1, [0, len(s1)], seed=seed)["loc"]
    w1 = ctx.scene_moments_fields(st1, p1, one["mean_field"][None], fields[m:m + 1])
    assert all(_eq(one[k], w1[k]) for k in KEYS)


# ---- 4: mask and edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_a_masked_pixel_reaches_nothing(cs, nb, F):
    names, stamps, places, fp, T, D = _host_scene(cs, nb, F)
    ctx = _ctx()
    plain = _host_gpu(cs, nb, F)
    ones = ctx.scene_moments_fields(stamps, places, T, D, weight_fields=np.ones_like(D), field_ptr=fp)
    for k in KEYS:
        assert _eq(ones[k], plain[k]), k                              # all-ones weights: the call without weights
    # a NaN, an inf and a huge value of D under weights of 0, a negative value, NaN and inf, in the crowded field and under the
    # galaxy alone in field 0; some bands only for two of them
    W, D2 = np.ones_like(D), D.copy()
    rng = np.random.default_rng(33)
    spots = [(0, int(places[0][0]) + cs // 2, int(places[0][1]) + cs // 2 + 1, slice(None))]
    spots += [(4, int(r), int(c), slice(None) if k % 2 else slice(1, 2)) for k, (r, c) in enumerate(rng.integers(2, F - 2, size=(11, 2)))]
    bad_w, bad_d = [0.0, -1.0, np.nan, np.inf], [np.nan, np.inf, 1e300, -np.inf]
    for k, (m, r, c, b) in enumerate(spots):
        W[m, r, c, b] = bad_w[k % 4]
        D2[m, r, c, b] = bad_d[(k + k // 4) % 4]
    on = mf.counts(W)
    D3 = np.where(on, D, T)                                           # the same scene with those pixels of D set to T
    masked = ctx.scene_moments_fields(stamps, places, T, D2, weight_fields=W, field_ptr=fp)
    clean = ctx.scene_moments_fields(stamps, places, T, D3, field_ptr=fp)
    for k in ("flux_data", "shape_data", "iters_data", "status_data"):
        assert _eq(masked[k], clean[k]), k
    assert np.isfinite(masked["flux_data"]).all()
    _, hidden = mf.child_images(stamps, places, fp, T, D, np.where(on, 0.0, 1.0))   # (counts the masked pixels of every stamp)
    drop = hidden.reshape(len(stamps), cs * cs, nb).sum(axis=1)
    assert np.array_equal(clean["npix_data"] - masked["npix_data"], drop) and drop[0].tolist() == [1] * nb and drop.sum() > nb
    # unmasked, one NaN of D under a counting pixel of `band` gives status 3 on exactly the rows whose stamp covers it
    m, r, c = 3, F // 2, F // 2
    D4 = D.copy()
    D4[m, r, c, 2] = np.nan
    hit = ctx.scene_moments_fields(stamps, places, T, D4, field_ptr=fp, band=2)
    p = np.asarray(places, dtype=np.int64)
    covers = np.zeros(len(stamps), dtype=bool)
    covers[fp[m]:fp[m + 1]] = ((p[fp[m]:fp[m + 1], 0] <= r) & (r < p[fp[m]:fp[m + 1], 0] + cs) &
                               (p[fp[m]:fp[m + 1], 1] <= c) & (c < p[fp[m]:fp[m + 1], 1] + cs))
    assert covers.sum() >= 1 and (hit["status_data"][covers] == 3).all()
    assert _eq(hit["status_data"][~covers], plain["status_data"][~covers]) and _eq(hit["shape_data"][~covers], plain["shape_data"][~covers])
    assert np.isnan(hit["flux_data"][covers, 2]).all() and _eq(hit["flux_data"][:, :2], plain["flux_data"][:, :2])
    # in another band the same NaN leaves the moments alone
    D4[m, r, c, 2], D4[m, r, c, 0] = D[m, r, c, 2], np.nan
    other = ctx.scene_moments_fields(stamps, places, T, D4, field_ptr=fp, band=2)
    assert _eq(other["shape_data"], plain["shape_data"]) and _eq(other["status_data"], plain["status_data"])


# ---- 5: DeblendFieldBatch ----------------------------------------------------------------------------------------------------
def test_deblend_field_batch_takes_the_moments_on_the_fields():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    fields = _blob_fields(3, F2, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-45, 46, size=(n, 2)).astype(np.float64) for n in (20, 0, 45)]
    sky = np.linspace(0.03, 0.06, 3 * NB).reshape(3, NB)
    W = np.ones_like(fields)
    W[:, 40:60, 50:80, :] = 0.0

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds
        return DeblendFieldBatch(net, fields, CS, NB)

    a, b, c, d = batch(), batch(), batch(), batch()
    res = a.deblend_fields(dists, on_device=True, measure=True, moments_data=True, moments_weights=W, sky_sigma=sky)
    plain = b.deblend_fields(dists, on_device=True, measure=True)
    host = c.deblend_fields(dists, measure=True)                  # the default path: stamps and catalogue on the host
    model = c.get_predicted_fields()["predicted_mean_fields"]
    names = tuple(n[0] for n in ms.moments_data_dtype(NB))
    want_cols = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + DeblendFieldBatch.moments_data_columns(NB))
    for m, (r, p, h) in enumerate(zip(res, plain, host)):
        assert r.dtype == want_cols and len(r) == len(p)
        for k in p.dtype.names:                                   # the columns of the call without it, value for value
            if k != "shifts":
                assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].base.kind == "f"), k
        if not len(r):
            continue
        mean = np.stack([np.asarray(x) for x in h["output_images_mean"]])
        places = int((F2 - CS) / 2) + dists[m].astype(np.int64)
        want = ms.measure_moments_on_fields(mean, places, fields[m], model[m], weight_fields=W[m], catalogue=h, sky_sigma=sky[m], ctx=c._ctx)
        for k in names:
            assert np.array_equal(r[k], want[k], equal_nan=True), (m, k)
        assert (r["npix_data"] < CS * CS).any() and np.array_equal(r["flux_data_err"], sky[m] * np.sqrt(r["npix_data"].astype(np.float64)))
        ok = r["status_data"] == 0
        assert np.isfinite(r["sigma_data"][ok]).all() and np.isnan(r["sigma_data"][r["status_data"] == 3]).all()
    cat = d.deblend_fields(dists, on_device=True, measure=True, moments_data=True, moments_weights=W, sky_sigma=sky, return_fields=False)
    for r, q in zip(res, cat):
        for k in r.dtype.names:
            if k != "shifts":
                assert np.array_equal(r[k], q[k], equal_nan=r.dtype[k].base.kind == "f"), k


# ---- against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.05, 0.1])
@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_scene_moments_fields_against_the_restatement(cs, nb, F, noise):
    """Synthetic galaxies: the scene of tests/test_gpu_fit_flux.py, whose data are the stamps at amplitudes 0.7 .. 1.3 plus noise
    0.05; the second draw adds noise up to 0.1"""
    names, stamps, places, fp, T, D = _host_scene(cs, nb, F)
    if noise == 0.05:
        got = _host_gpu(cs, nb, F)
    else:
        D = D + np.random.default_rng(600 + cs).normal(0.0, np.sqrt(noise ** 2 - 0.05 ** 2), size=D.shape)
        got = _ctx().scene_moments_fields(stamps, places, T, D, field_ptr=fp)
    _against_the_restatement(f"{cs}/{nb}/{F} noise {noise}", got, stamps, places, fp, T, D)
    out_rows = [i for i, n in enumerate(names) if n == "outside"]
    assert (got["npix_data"][out_rows] == 0).all()                   # a stamp wholly outside gets the model's row
    model = _ctx().scene_measure(stamps[out_rows], None)
    assert _eq(got["shape_data"][out_rows], model["shape"]) and _eq(got["flux_data"][out_rows], model["flux"])


@pytest.mark.parametrize("noise", [0.05, 0.1])
def test_network_stamps_on_blob_fields_against_the_restatement(noise):
    """The network's own stamps and composite on _blob_fields (noise 0.05), and a second draw with noise 0.1, with weights"""
    net, fields, starts, places, fp, stamps, T = _network_scene("float32")
    D, W = fields, None
    if noise != 0.05:
        rng = np.random.default_rng(17)
        D = fields + rng.normal(0.0, np.sqrt(noise ** 2 - 0.05 ** 2), size=fields.shape)
        W = np.where(rng.random(fields.shape) < 0.05, 0.0, 1.0)
    got = net._core.ctx.scene_moments_fields(stamps, places, T, D, weight_fields=W, field_ptr=fp)
    _against_the_restatement(f"network 31/{NB}/{F2} noise {noise}", got, stamps, places, fp, T, D, W)


# ---- the purpose -------------------------------------------------------------------------------------------------------------
def test_a_round_model_does_not_bias_the_shape_measured_on_the_data():
    """D = G1 + G2: G1 an elliptical Gaussian of sigma 2.5 and |e| = 0.3, G2 a round one of sigma 2, 25.4 px away - the two
    31-pixel stamps overlap by 15 x 11 pixels and G2's light reaches into the corner of stamp 1, but what the wrong model of
    galaxy 1 leaves under galaxy 2's weight is below 1e-10 of galaxy 2's light.  The models: P2 = G2 cast to float32, P1 a round Gaussian of sigma 3.0 at G1's place, T = P1 + P2."""
    from debvader_amd.measure import measurement as ms

    cs, nb, F = 31, 3, 64
    tr = 2.0 * 6.25 / np.sqrt(1.0 - 0.3 ** 2)                       # sigma^2 = sqrt(det) = (tr / 2) sqrt(1 - e^2)
    e1, e2 = 0.24, 0.18
    M1 = (0.5 * tr * (1.0 - e1), 0.5 * tr * e2, 0.5 * tr * (1.0 + e1))
    bands = np.array([0.6, 0.8, 1.0])
    o1, o2 = (0.3, -0.2), (-0.4, 0.1)
    places = np.array([[8, 6], [24, 26]], np.int32)
    rr, cc = np.arange(F, dtype=np.float64)[:, None], np.arange(F, dtype=np.float64)[None, :]

    def on_field(M, place, off, amp):
        r, c = rr - (place[0] + 15.0 + off[0]), cc - (place[1] + 15.0 + off[1])
        det = M[0] * M[2] - M[1] * M[1]
        return amp * np.exp(-0.5 * (M[2] * r * r - 2.0 * M[1] * r * c + M[0] * c * c) / det)

    G1, G2 = on_field(M1, places[0], o1, 1.0), on_field((4.0, 0.0, 4.0), places[1], o2, 0.8)
    D = ((G1 + G2)[:, :, None] * bands)[None]
    P1 = (mo.gaussian_stamp(cs, (9.0, 0.0, 9.0), o1)[:, :, None] * bands).astype(np.float32)
    P2 = (G2[24:55, 26:57, None] * bands).astype(np.float32)
    stamps = np.stack([P1, P2])
    T = _composite(stamps, places, [0, 2], F)
    ctx = _ctx()
    got = ctx.scene_moments_fields(stamps, places, T, D)
    model = ctx.scene_measure(stamps, None)
    assert (got["status_data"] == 0).all() and (model["status"] == 0).all()
    # galaxy 1: the moments of G1 + (G2 - (double)P2), the float32 rounding of P2 left in
    child1 = (G1 + G2)[8:39, 6:37] * bands[2]
    child1[16:, 20:] -= P2[:15, :11, 2].astype(np.float64)
    want, _, st = mo.adaptive_moments(child1)
    assert st == 0 and np.abs(got["shape_data"][0] - want).max() < 1e-6
    rec = ms.moments_data_records(*(got[k] for k in KEYS))
    cat = ms.catalogue_records(model["flux"], None, model["shape"], model["iters"], model["status"])
    print(f"galaxy 1: model e = ({cat['e1'][0]:+.2e}, {cat['e2'][0]:+.2e}) sigma {cat['sigma'][0]:.4f}; on the data e = "
          f"({rec['e1_data'][0]:+.6f}, {rec['e2_data'][0]:+.6f}) sigma {rec['sigma_data'][0]:.4f}; G1 has ({e1}, {e2}) and 2.5")
    assert abs(cat["e1"][0]) < 1e-6 and abs(cat["e2"][0]) < 1e-6 and abs(cat["sigma"][0] - 3.0) < 1e-3
    assert abs(rec["e1_data"][0] - cat["e1"][0] - e1) < 1e-4 and abs(rec["e2_data"][0] - cat["e2"][0] - e2) < 1e-4
    assert abs(rec["sigma_data"][0] - 2.5) < 1e-4
    # galaxy 2's model was right: its row on the data is its model row
    assert np.abs(got["shape_data"][1] - model["shape"][1]).max() < 1e-6
    # G2's light in the corner of stamp 1 is subtracted: the flux on the data is G1's, not the model's and not G1 + G2's
    assert np.abs(got["flux_data"][0] - G1[8:39, 6:37].sum() * bands).max() < 1e-5
    assert G2[8:39, 6:37].sum() > 0.01 and abs(model["flux"][0, 2] - G1[8:39, 6:37].sum()) > 10.0


# ---- sizes where the kernel can go wrong -------------------------------------------------------------------------------------
def _small(cs, nb, F, counts, seed, noise=0.03):
    """galaxies of sigma 1.8 .. 3.5 px (scaled to the stamp) in fields of F pixels, some over the edges: (stamps, places, fp, T, D)"""
    rng = np.random.default_rng(seed)
    n = int(np.sum(counts))
    s = min(1.0, cs / 31.0)
    stamps = np.zeros((n, cs, cs, nb), np.float32)
    for i in range(n):
        a, b = (rng.uniform(1.8, 3.5, size=2) * s) ** 2
        M = (a, rng.uniform(-0.4, 0.4) * np.sqrt(a * b), b)
        stamps[i] = (mo.gaussian_stamp(cs, M, rng.uniform(-1.0, 1.0, size=2) * s, rng.uniform(0.8, 2.0))[:, :, None] *
                     rng.uniform(0.5, 1.0, size=nb)).astype(np.float32)
    places = rng.integers(-cs // 3, max(F - cs + cs // 3, 1), size=(n, 2)).astype(np.int32)
    fp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    T = _composite(stamps, places, fp, F)
    D = 1.1 * T + rng.normal(0.0, noise, size=T.shape)
    return stamps, places, fp, T, D


@pytest.mark.parametrize("cs,nb,band,F,counts", [(16, 3, 2, 40, [5, 0, 4]), (17, 3, 1, 40, [4, 0, 5]), (31, 1, 0, 50, [6]),
                                                 (31, 15, 14, 50, [3, 3]), (17, 2, 1, 10, [4])])
def test_sizes_where_the_kernel_can_go_wrong(cs, nb, band, F, counts):
    """cs = 16 (a whole number of stamp rows per 256 threads) and 17; one band with band 0 and fifteen with band 14; a field
    smaller than the stamp; a field with no galaxies between two that have some"""
    stamps, places, fp, T, D = _small(cs, nb, F, counts, seed=100 + cs + nb)
    ctx = _ctx()
    same = ctx.scene_moments_fields(stamps, places, T, T, field_ptr=fp, band=band)
    want = ctx.scene_measure(stamps, None, band=band)
    for a, b in (("shape_data", "shape"), ("iters_data", "iters"), ("status_data", "status"), ("flux_data", "flux")):
        assert _eq(same[a], want[b]), a
    got = ctx.scene_moments_fields(stamps, places, T, D, field_ptr=fp, band=band)
    W = np.where(np.random.default_rng(3).random(D.shape) < 0.1, 0.0, 2.0)
    gotw = ctx.scene_moments_fields(stamps, places, T, D, weight_fields=W, field_ptr=fp, band=band)
    if F < cs:
        assert (got["npix_data"] <= F * F).all() and (got["npix_data"] > 0).all()
    _against_the_restatement(f"{cs}/{nb}/{F}", got, stamps, places, fp, T, D, band=band)
    _against_the_restatement(f"{cs}/{nb}/{F} weighted", gotw, stamps, places, fp, T, D, W, band=band)
    # N = 0 returns at once
    empty = ctx.scene_moments_fields(stamps[:0], places[:0], T, D, field_ptr=np.zeros(len(fp), np.int64), band=band)
    assert all(empty[k].shape[0] == 0 for k in KEYS)


def test_the_largest_stamp_and_the_first_that_is_refused():
    from debvader_amd import _lib
    from debvader_amd.engine import _dp, _fp, _ip

    cs, F = 90, 120
    stamps, places, fp, T, D = _small(cs, 1, F, [3], seed=9)
    ctx = _ctx()
    got = ctx.scene_moments_fields(stamps, places, T, D, band=0)
    _against_the_restatement("90/1/120", got, stamps, places, fp, T, D, band=0)
    same = ctx.scene_moments_fields(stamps, places, T, T, band=0)
    assert _eq(same["shape_data"], ctx.scene_measure(stamps, None, band=0)["shape"])
    # 91 pixels: refused by name before any GPU work, by the wrapper and by the library; the next call gives the same bits
    big = np.zeros((1, 91, 91, 1), np.float32)
    with pytest.raises(ValueError, match="stamps of 91 pixels: the measurement takes at most 90"):
        ctx.scene_moments_fields(big, places[:1], T, D, band=0)
    par = _lib.DvMeasureParams(0, 3.0, 1e-10, 200)
    out = [np.zeros((1, 1)), np.zeros((1, 1), np.int32), np.zeros((1, 5)), np.zeros(1, np.int32), np.zeros(1, np.int32)]
    fq = np.array([0, 1], np.int64)
    with pytest.raises(_lib.DvError, match="dv_scene_moments_fields: the 91 x 91 band plane.*stamps of at most 90 pixels"):
        _lib.check(_lib.lib.dv_scene_moments_fields(ctx._h, _fp(big), _ip(np.ascontiguousarray(places[:1])),
                                                    fq.ctypes.data_as(C.POINTER(C.c_int64)), 1, 91, 1, _dp(T), _dp(D), None, 1, F,
                                                    C.byref(par), _dp(out[0]), _ip(out[1]), _dp(out[2]), _ip(out[3]), _ip(out[4])))
    again = ctx.scene_moments_fields(stamps, places, T, D, band=0)
    for k in KEYS:
        assert _eq(again[k], got[k]), k


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_gpu_work_and_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import Engine, _dp, _fp, _ip

    DvError, lib = _lib.DvError, _lib.lib
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(1, F2, seed=11)
    starts, places, fp = _windows(F2, [5], seed=5, hang=False)
    good = eng.infer_fields_measure_moments_data(fields, starts, fp, places, seed=3)

    n, nb = 5, NB
    ptr = lambda a: None if a is None else (_dp(a) if a.dtype == np.float64 else _fp(a) if a.dtype == np.float32 else _ip(a))   # noqa: E731
    cat = [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    five = lambda n, nb: [np.zeros((n, nb)), np.zeros((n, nb), np.int32), np.zeros((n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)]   # noqa: E731
    md = five(n, nb)
    f2, N, args = Engine._field_args(fields, starts, fp, places)
    mean_f, std_f, res_f = np.empty(f2.shape), np.empty(f2.shape), np.empty(f2.shape)

    def pipeline(par=None, out=None, fields_out=(None, None, None), no_params=False, no_places=False, a=None, weights=None):
        par = par or _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
        a = list(args if a is None else a)
        if no_places:
            a[5] = None
        _lib.check(lib.dv_infer_fields_measure_moments_data(eng._h, *a, 9, None if no_params else C.byref(par), *fields_out, None,
                                                            *map(ptr, cat), ptr(weights), *map(ptr, md if out is None else out)))

    P, pl = np.ones((3, 31, 31, 3), np.float32), np.zeros((3, 2), np.int32)
    T, D = np.zeros((2, 40, 40, 3)), np.ones((2, 40, 40, 3))
    md2 = five(3, 3)

    def scene(stamps=P, places=pl, fptr=(0, 2, 3), n=3, cs=31, nb=3, model=T, data=D, weights=None, M=2, F=40, par=None, out=None,
              no_params=False):
        par = par or _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
        fptr = None if fptr is None else np.asarray(fptr, np.int64)
        _lib.check(lib.dv_scene_moments_fields(ctx._h, ptr(stamps), ptr(places),
                                               None if fptr is None else fptr.ctypes.data_as(C.POINTER(C.c_int64)), n, cs, nb,
                                               ptr(model), ptr(data), ptr(weights), M, F, None if no_params else C.byref(par),
                                               *map(ptr, md2 if out is None else out)))

    with pytest.raises(DvError, match="dv_scene_moments_fields: params must be given"):
        scene(no_params=True)
    with pytest.raises(DvError):
        pipeline(no_params=True)
    for call, who in ((pipeline, "dv_infer_fields_measure_moments_data"), (scene, "dv_scene_moments_fields")):
        for par, msg in ((_lib.DvMeasureParams(NB, 3.0, 1e-10, 200), "band"), (_lib.DvMeasureParams(-1, 3.0, 1e-10, 200), "band"),
                         (_lib.DvMeasureParams(2, 0.0, 1e-10, 200), "sigma0"), (_lib.DvMeasureParams(2, float("nan"), 1e-10, 200), "sigma0"),
                         (_lib.DvMeasureParams(2, 3.0, 0.0, 200), "tol"), (_lib.DvMeasureParams(2, 3.0, 1e-10, -1), "max_iter")):
            with pytest.raises(DvError, match=who + ".*" + msg):
                call(par=par)
        for k in range(5):                                        # a missing output
            out = list(md if call is pipeline else md2)
            out[k] = None
            with pytest.raises(DvError, match=who + ": flux_data, npix_data, shape_data, iters_data and status_data must all be given"):
                call(out=out)
    # the pipeline: a null places in both forms, what dv_infer_fields_measure refuses
    with pytest.raises(DvError, match="places"):
        pipeline(no_places=True)
    with pytest.raises(DvError, match="places"):
        pipeline(no_places=True, fields_out=(_dp(mean_f), _dp(std_f), None))
    with pytest.raises(DvError, match="go together"):
        pipeline(fields_out=(_dp(mean_f), None, None))
    # the host call: its inputs, the field table, the placements, the sizes
    for kw, msg in ((dict(stamps=None), "must all be given"), (dict(places=None), "must all be given"),
                    (dict(model=None), "must all be given"), (dict(data=None), "must all be given"),
                    (dict(fptr=None), "must all be given"), (dict(n=-1), "must all be given"), (dict(M=-1), "must all be given"),
                    (dict(fptr=(1, 2, 3)), "field_ptr must run from 0"), (dict(fptr=(0, 2, 4)), "field_ptr must run from 0"),
                    (dict(fptr=(0, 4, 3)), "decreases at field 1"), (dict(fptr=(0, -1, 3)), "decreases at field 0"),
                    (dict(places=np.array([[0, 0], [1 << 29, 0], [0, 0]], np.int32)), "placement 1"),
                    (dict(places=np.array([[0, 0], [0, 0], [0, -(1 << 29)]], np.int32)), "placement 2"),
                    (dict(F=0), "fields of 0 pixels"), (dict(F=40000), "fields of 40000 pixels"),
                    (dict(cs=0), "stamps of 0 pixels"), (dict(cs=91), "stamps of at most 90 pixels"),
                    (dict(nb=17), "17 bands"), (dict(nb=0), "0 bands")):
        with pytest.raises(DvError, match="dv_scene_moments_fields: .*" + msg):
            scene(**kw)
    # every refusal left the stream idle: nothing is queued, and the context answers at once
    ctx.sync()
    # nothing to do with N = 0; a correct call runs: three stamps of ones on data of ones over a model of zeros
    scene(n=0, fptr=(0, 0, 0), stamps=None, places=None, model=None, data=None, out=[None] * 5)
    scene()
    assert (md2[0] == 2.0 * 961.0).all() and (md2[1] == 961).all() and (md2[4] == md2[4][0]).all()
    scene(weights=np.zeros((2, 40, 40, 3)))                       # wholly masked: the model's row
    assert (md2[0] == 961.0).all() and (md2[1] == 0).all()
    # the engine completes a correct call afterwards, with the bits it gave before
    again = eng.infer_fields_measure_moments_data(fields, starts, fp, places, seed=3)
    for k in good:
        assert _eq(again[k], good[k]), k
    pipeline(fields_out=(_dp(mean_f), _dp(std_f), _dp(res_f)))
    assert np.array_equal(mean_f, eng.infer_fields_composite(fields, starts, places, fp, seed=9)["mean_fields"])
    ref = eng.infer_fields_measure_moments_data(fields, starts, fp, places, seed=9)
    assert all(_eq(a, ref[k]) for a, k in zip(md, KEYS))
