"""The flux fit by blend groups on the GPU (dv_scene_fit_flux_groups, dv_scene_fit_groups).  The groups
are compared with the union-find restatement of tests/fit_flux_groups_oracle.py, exactly.  The fit is compared with the dense
calls BIT FOR BIT wherever they take the field: galaxies of different groups share no term, so the dense factorisation applies
to every element exact zeros of the other groups' columns (x - 0 y has the bits of x for finite y), h' subtracts exact zeros,
the sums of squares of L^-1 add exact zeros in ascending order, and the chi-square walks the same ascending neighbour list.
Beyond the dense limit there is no dense call on the whole field: the reference is the dense call on the clusters as fields of
their own, again bit for bit, and the bounds of tests/test_gpu_fit_flux.py against numpy on the GPU's own Gram blocks."""
import functools

import numpy as np
import pytest

from tests import fit_flux_groups_oracle as go
from tests import fit_flux_oracle as fo
from tests.test_gpu_fit_flux import SHAPES, _scene

pytestmark = pytest.mark.gpu

KEYS = ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status")
WKEYS = KEYS + ("fit_chi2", "fit_npix")
GKEYS = ("fit_group", "fit_group_size")


def _ctx():
    from debvader_amd import engine as E

    return E.default_context()


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _frozen(out):
    for a in out.values():
        a.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def _weights(cs, nb, F):
    """weight fields of the scene: inverse variances around 1 with a block of zeros, a NaN, an inf and a negative value in
    every field, all under stamps of the crowds"""
    rng = np.random.default_rng(700 + cs)
    W = rng.uniform(0.5, 2.0, size=(6, F, F, nb))
    W[:, F // 3:F // 3 + 5, F // 4:F // 4 + 7] = 0.0
    W[:, F // 2, F // 2, 0] = np.nan
    W[:, F // 2 + 1, F // 2, nb - 1] = np.inf
    W[:, F // 2, F // 2 + 2] = -1.0
    W.flags.writeable = False
    return W


@functools.lru_cache(maxsize=None)
def _dense(cs, nb, F, weighted):
    _, stamps, places, fp, D = _scene(cs, nb, F)
    return _frozen(_ctx().scene_fit_flux(stamps, places, D, field_ptr=fp, weight_fields=_weights(cs, nb, F) if weighted else None))


@functools.lru_cache(maxsize=None)
def _grouped(cs, nb, F, weighted):
    _, stamps, places, fp, D = _scene(cs, nb, F)
    return _frozen(_ctx().scene_fit_flux_groups(stamps, places, D, field_ptr=fp,
                                                weight_fields=_weights(cs, nb, F) if weighted else None))


@functools.lru_cache(maxsize=None)
def _scene_groups(cs, nb, F):
    _, _, places, fp, _ = _scene(cs, nb, F)
    return go.groups(places, fp, cs, F)


# ---- 1: the bits of the dense fit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_the_grouped_fit_has_the_bits_of_the_dense_fit(cs, nb, F, weighted):
    names, stamps, places, fp, D = _scene(cs, nb, F)
    want, got = _dense(cs, nb, F, weighted), _grouped(cs, nb, F, weighted)
    keys = WKEYS if weighted else KEYS
    assert sorted(got) == sorted(keys + GKEYS)
    assert np.isfinite(want["fit_scale"]).any() and np.isnan(want["fit_scale"]).any() and (want["fit_status"] == 5).any()
    for k in keys:
        assert _eq(got[k], want[k]), k
    group, size = _scene_groups(cs, nb, F)
    assert _eq(got["fit_group"], group) and _eq(got["fit_group_size"], size)
    # what the scene holds (its fields are two stamps wide, so the rectangles of a crowd all touch): the fields of one galaxy are
    # singletons, the two stamps wholly outside are groups of their own, everybody else of the crowd - the duplicate and the
    # all-zero stamp, which is ineligible and still a member, included - is one group, and so is the crowded field
    crowd = np.arange(int(fp[3]), int(fp[4]))
    outside = np.array([n == "outside" for n in names[crowd[0]:crowd[-1] + 1]])
    assert (size[crowd[outside]] == 1).all() and (group[crowd[outside]] == crowd[outside] - fp[3]).all()
    assert (size[crowd[~outside]] == 26).all() and (group[crowd[~outside]] == 0).all() and outside.sum() == 2
    assert size[0] == 1 and size[1] == 1 and size[-1] == 1 and (size[fp[4]:fp[5]] == 40).all()


# ---- 2: beyond the dense limit ------------------------------------------------------------------------------------------------
NCL, PER = 5, 260


@functools.lru_cache(maxsize=None)
def _clusters():
    """1300 stamps of 9 pixels, one band, in a field of 200: five clusters of 260 on a 3-pixel grid (20 x 13 cells, the recipe of
    test_a_field_of_more_galaxies_than_threads) in five areas more than a stamp apart, the rows interleaved round-robin"""
    cs, F = 9, 200
    rng = np.random.default_rng(19)
    cells = np.arange(PER)
    origins = [(0, 0), (0, 60), (0, 120), (80, 0), (80, 60)]
    places = np.zeros((PER, NCL, 2), np.int32)                       # row k NCL + c of the call: cell k of cluster c
    for c, (r0, c0) in enumerate(origins):
        places[:, c] = np.stack([r0 + (cells // 13) * 3, c0 + (cells % 13) * 3], axis=1)
    places = places.reshape(-1, 2)
    n = len(places)
    stamps = np.stack([fo.elliptical_gaussian(cs, (1.4, rng.uniform(-0.3, 0.3), 1.4), rng.uniform(-0.5, 0.5, 2), rng.uniform(0.5, 2.0))
                       for _ in range(n)])[..., None].astype(np.float32)
    D = rng.normal(0.0, 0.05, size=(F, F, 1))
    for i in range(n):
        ra, rz, ca, cz = fo.clip(places[i], cs, F)
        D[ra:rz, ca:cz] += stamps[i, ra - places[i, 0]:rz - places[i, 0], ca - places[i, 1]:cz - places[i, 1]].astype(np.float64)
    for a in (stamps, places, D):
        a.flags.writeable = False
    return cs, F, stamps, places, D


def test_a_field_beyond_the_dense_limit():
    from debvader_amd._lib import DvError

    cs, F, stamps, places, D = _clusters()
    n = len(places)
    ctx = _ctx()
    # every cluster as a field of its own over the same data field: the dense call takes that
    order = np.concatenate([np.arange(c, n, NCL) for c in range(NCL)])
    fp = np.arange(NCL + 1) * PER
    dense = ctx.scene_fit_flux(stamps[order], places[order], np.broadcast_to(D, (NCL, F, F, 1)), field_ptr=fp)
    blocks = []
    for c in range(NCL):
        rows = order[c * PER:(c + 1) * PER]
        g = ctx.scene_fit_flux_gram(stamps[rows], places[rows], D)
        A = np.tril(g["gram"][0]) + np.tril(g["gram"][0], -1).T
        d = 1.0 / np.sqrt(np.diagonal(A))
        cond = np.linalg.cond(A * d[:, None] * d[None, :])
        print(f"cluster {c}: scaled condition number {cond:.1f}")
        assert cond < 100.0                                          # the precondition of the bounds below
        blocks.append((rows, A, g["proj"][:, 0]))
    with pytest.raises(DvError, match="field 0 has 1300 galaxies, the dense fit takes at most 1024"):
        ctx.scene_fit_flux(stamps, places, D[None])
    got = ctx.scene_fit_flux_groups(stamps, places, D[None])
    assert got["fit_group"].tolist() == (np.arange(n) % NCL).tolist() and (got["fit_group_size"] == PER).all()
    assert (got["fit_status"] == 0).all()
    for k in KEYS:
        assert _eq(got[k][order], dense[k]), k
    worst = dict(backward=0.0, scale=0.0, var=0.0)
    for rows, A, h in blocks:
        assert np.array_equal(np.diagonal(A), got["fit_gram"][rows, 0]) and np.array_equal(h, got["fit_proj"][rows, 0])
        a, v = got["fit_scale"][rows, 0], got["fit_var"][rows, 0]
        want, wv = np.linalg.solve(A, h), np.diagonal(np.linalg.inv(A))
        back, bound = np.abs(A @ a - h).max(), 1e-10 * (np.abs(A).sum(axis=1).max() * np.abs(a).max() + np.abs(h).max())
        worst["backward"] = max(worst["backward"], back / bound)
        worst["scale"] = max(worst["scale"], np.abs(a - want).max() / (1e-10 * np.abs(want).max()))
        worst["var"] = max(worst["var"], (np.abs(v - wv) / wv).max() / 1e-9)
        assert back <= bound
        assert (np.abs(a - want) <= 1e-10 * np.abs(want).max()).all() and (np.abs(v - wv) <= 1e-9 * wv).all()
    print("1300 galaxies in five groups of 260: worst fraction of each bound - " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ---- 3: labels that must travel -----------------------------------------------------------------------------------------------
def _blobs(n, cs, seed):
    rng = np.random.default_rng(seed)
    return np.stack([fo.elliptical_gaussian(cs, (1.4, rng.uniform(-0.3, 0.3), 1.4), rng.uniform(-0.5, 0.5, 2), rng.uniform(0.5, 2.0))
                     for _ in range(n)])[..., None].astype(np.float32)


def test_labels_that_must_travel():
    cs, F, n = 9, 300, 600
    rng = np.random.default_rng(5)
    path = go.serpentine(n, cs, F)
    pos = rng.permutation(n)                                         # row r of the field sits at position pos[r] of the path
    pos[np.nonzero(pos == 0)[0][0]], pos[0] = pos[0], 0              # the smallest row at one end
    chain = path[pos]
    side = 6 * (cs - 1)
    ring = np.array([(0, 8 * i) for i in range(7)] + [(8 * i, side) for i in range(1, 7)] +
                    [(side, side - 8 * i) for i in range(1, 7)] + [(side - 8 * i, 0) for i in range(1, 6)], np.int32) + 20
    # two chains along the upper edge, partly outside it; between them a stamp that touches both by one pixel column: clipped by
    # the edge it joins them, wholly outside (its rectangle still meets theirs above the field) it does not
    two = [(-4, 0), (-4, 8), (-4, 16), (-4, 32), (-4, 40)]
    bridged = np.array(two + [(-6, 24)], np.int32)
    apart = np.array(two + [(-9, 24)], np.int32)
    places = np.concatenate([chain, ring, bridged, apart])
    fp = np.cumsum([0, n, len(ring), len(bridged), len(apart)])
    want_g, want_s = go.groups(places, fp, cs, F)
    assert (want_s[:n] == n).all() and (want_g[:n] == 0).all() and (want_s[n:n + 24] == 24).all()
    assert want_s[fp[2]:fp[3]].tolist() == [6] * 6 and want_s[fp[3]:].tolist() == [3, 3, 3, 2, 2, 1]
    ctx = _ctx()
    got = ctx.scene_fit_groups(places, cs, F, field_ptr=fp, lists=True)
    assert _eq(got["fit_group"], want_g) and _eq(got["fit_group_size"], want_s)
    pairs, adj_ptr, adj = go.lists(places, fp, cs, F)
    assert _eq(got["pairs"], pairs) and _eq(got["adj_ptr"], adj_ptr) and _eq(got["adj"], adj)
    again = ctx.scene_fit_groups(places, cs, F, field_ptr=fp, lists=True)
    assert all(_eq(again[k], got[k]) for k in got)
    # the fit gives the same groups, and one band of a chain is a system like any other
    stamps = _blobs(len(places), cs, 6)
    D = rng.normal(0.0, 0.05, size=(4, F, F, 1))
    fit = ctx.scene_fit_flux_groups(stamps, places, D, field_ptr=fp)
    assert _eq(fit["fit_group"], want_g) and _eq(fit["fit_group_size"], want_s)
    dense = ctx.scene_fit_flux(stamps, places, D, field_ptr=fp)
    for k in KEYS:
        assert _eq(fit[k], dense[k]), k
    assert fit["fit_status"][-1, 0] == 4 and (fit["fit_status"][:n] == 0).all()


# ---- 4: the group limit -------------------------------------------------------------------------------------------------------
def test_the_group_limit():
    from debvader_amd._lib import DvError

    cs, F, many = 9, 400, 1025
    path = go.serpentine(many, cs, F)
    stamps = _blobs(1 + many, cs, 8)
    rng = np.random.default_rng(3)
    D = rng.normal(0.0, 0.05, size=(2, F, F, 1))
    for i in range(many):
        ra, rz, ca, cz = fo.clip(path[i], cs, F)
        D[1, ra:rz, ca:cz] += stamps[1 + i].astype(np.float64)
    places = np.concatenate([[[5, 5]], path]).astype(np.int32)
    ctx = _ctx()
    n = many - 1
    before = ctx.scene_fit_flux_groups(stamps[:1 + n], places[:1 + n], D, field_ptr=[0, 1, 1 + n])
    assert before["fit_group_size"].tolist() == [1] + [n] * n and (before["fit_status"] == 0).all()
    g = ctx.scene_fit_flux_gram(stamps[1:1 + n], places[1:1 + n], D[1])
    A = np.tril(g["gram"][0]) + np.tril(g["gram"][0], -1).T
    a, h = before["fit_scale"][1:, 0], g["proj"][:, 0]
    assert np.array_equal(h, before["fit_proj"][1:, 0])
    back, bound = np.abs(A @ a - h).max(), 1e-10 * (np.abs(A).sum(axis=1).max() * np.abs(a).max() + np.abs(h).max())
    print(f"a chain of {n}: fraction of the backward-error bound {back / bound:.1e}")
    assert back <= bound and np.abs(a - 1.0).max() < 0.5
    with pytest.raises(DvError, match=r"dv_scene_fit_flux_groups: field 1: the blend group of row 0 has 1025 galaxies, the grouped "
                                      r"fit takes at most 1024 per group"):
        ctx.scene_fit_flux_groups(stamps, places, D, field_ptr=[0, 1, 1 + many])
    after = ctx.scene_fit_flux_groups(stamps[:1 + n], places[:1 + n], D, field_ptr=[0, 1, 1 + n])
    assert all(_eq(after[k], before[k]) for k in before)


# ---- 5: rows keep their bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs,nb,F", SHAPES)
def test_rows_keep_their_bits(cs, nb, F):
    from debvader_amd._lib import DvError

    _, stamps, places, fp, D = _scene(cs, nb, F)
    W = _weights(cs, nb, F)
    ctx = _ctx()
    got = _grouped(cs, nb, F, True)
    keys = WKEYS + GKEYS
    again = ctx.scene_fit_flux_groups(stamps, places, D, field_ptr=fp, weight_fields=W)
    for k in keys:
        assert _eq(again[k], got[k]), k
    order = np.concatenate([np.arange(fp[m], fp[m + 1]) for m in range(5, -1, -1)])
    fp_r = np.concatenate([[0], np.cumsum(np.diff(fp)[::-1])])
    moved = ctx.scene_fit_flux_groups(stamps[order], places[order], D[::-1], field_ptr=fp_r, weight_fields=W[::-1])
    for k in keys:
        assert _eq(moved[k], got[k][order]), k
    for m in (0, 3, 4):
        lo, hi = int(fp[m]), int(fp[m + 1])
        one = ctx.scene_fit_flux_groups(stamps[lo:hi], places[lo:hi], D[m:m + 1], weight_fields=W[m:m + 1])
        for k in keys:
            assert _eq(one[k], got[k][lo:hi]), (m, k)
    # a scratch that holds the largest group and no more: the groups go through it in several sub-ranges
    group, size = _scene_groups(cs, nb, F)
    big = int(size.max())
    tight = nb * big * big * 8
    roots = group == np.arange(len(group)) - fp[np.searchsorted(fp, np.arange(len(group)), "right") - 1]
    assert nb * 8 * int((size[roots].astype(np.int64) ** 2).sum()) > tight
    split = ctx.scene_fit_flux_groups(stamps, places, D, field_ptr=fp, weight_fields=W, scratch_bytes=tight)
    for k in keys:
        assert _eq(split[k], got[k]), k
    at = int(np.nonzero(size == big)[0][0])
    m = int(np.searchsorted(fp, at, "right") - 1)
    with pytest.raises(DvError, match=rf"field {m}: the blend group of row {at - int(fp[m])} has {big} galaxies.*{tight} bytes of "
                                      rf"scratch.*scratch_bytes is {tight - 1}"):
        ctx.scene_fit_flux_groups(stamps, places, D, field_ptr=fp, weight_fields=W, scratch_bytes=tight - 1)
    again = ctx.scene_fit_flux_groups(stamps, places, D, field_ptr=fp, weight_fields=W)
    for k in keys:
        assert _eq(again[k], got[k]), k


# ---- 6: the pipeline, both engines --------------------------------------------------------------------------------------------
F2 = 131


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_host_call(dtype, monkeypatch):
    from tests.test_gpu_aperture import CAT, COUNTS, CS, NB, _blob_fields, _net, _windows
    from tests.test_gpu_fit_flux_weighted import _draw_weights, _spoil

    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(5, F2, seed=11)
    starts, places, fp = _windows(F2, COUNTS, seed=5)
    rng = np.random.default_rng(7100 + CS)
    W, _ = _spoil(rng, _draw_weights(rng, fields.shape, CS), fields)
    seed = 77
    stamps = eng.infer_fields_keep(fields, starts, fp, seed=seed)["loc"]
    rows = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    fb = F2 * F2 * NB * 8
    for weights, keys, mb_fields, mb_only in ((None, KEYS + GKEYS, "10", ("5", "3")), (W, WKEYS + GKEYS, "13", ("5",))):
        want = ctx.scene_fit_flux_groups(stamps, places, fields, field_ptr=fp, weight_fields=weights)
        dense = ctx.scene_fit_flux(stamps, places, fields, field_ptr=fp, weight_fields=weights)
        assert all(_eq(want[k], dense[k]) for k in dense) and (want["fit_status"] == 0).any()
        assert want["fit_group_size"].max() > 1 and len(np.unique(want["fit_group_size"])) > 1
        got = eng.infer_fields_measure_fit_groups(fields, starts, fp, places, weight_fields=weights, seed=seed)
        assert sorted(got) == sorted(tuple(rows) + keys)
        for k in keys:
            assert _eq(got[k], want[k]), k
        for k in rows:                                            # every shared output has infer_fields_measure's bits
            assert _eq(got[k], rows[k]), k
        only = eng.infer_fields_measure_fit_groups(fields, starts, fp, places, weight_fields=weights, seed=seed, return_fields=False)
        assert sorted(only) == sorted(CAT + ("mse_center",) + keys)
        for k in only:
            assert _eq(only[k], got[k]), k
        # the group boundaries of the dense pipeline tests: three resident fields, so field 2 (stamps 30 .. 179, chunks of 64) is
        # carried from the first group of resident fields into the second and its fit runs there
        per = (5 if weights is not None else 4) * fb
        assert 3 * per <= int(mb_fields) << 20 < 4 * per
        monkeypatch.setenv("DV_FIELDS_GROUP_MB", mb_fields)
        carried = eng.infer_fields_measure_fit_groups(fields, starts, fp, places, weight_fields=weights, seed=seed)
        for k in got:
            assert _eq(carried[k], got[k]), k
        for mb in mb_only:
            monkeypatch.setenv("DV_FIELDS_GROUP_MB", mb)
            g2 = eng.infer_fields_measure_fit_groups(fields, starts, fp, places, weight_fields=weights, seed=seed, return_fields=False)
            for k in only:
                assert _eq(g2[k], only[k]), (mb, k)
        monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    # a scratch that takes the largest group alone: several sub-ranges at the seam, the same bits
    big = int(want["fit_group_size"].max())
    tight = eng.infer_fields_measure_fit_groups(fields, starts, fp, places, weight_fields=W, seed=seed, return_fields=False,
                                                scratch_bytes=NB * big * big * 8)
    for k in only:
        assert _eq(tight[k], only[k]), k


def test_deblend_field_batch_takes_the_groups():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms
    from tests.test_gpu_aperture import CS, NB, _blob_fields, _net

    fields = _blob_fields(3, F2, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-45, 46, size=(n, 2)).astype(np.float64) for n in (20, 0, 45)]
    sky = np.linspace(0.03, 0.06, 3 * NB).reshape(3, NB)

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds
        return DeblendFieldBatch(net, fields, CS, NB)

    a, b, c, d = batch(), batch(), batch(), batch()
    res = a.deblend_fields(dists, on_device=True, measure=True, fit_flux=True, fit_groups=True, sky_sigma=sky)
    dense = b.deblend_fields(dists, on_device=True, measure=True, fit_flux=True, sky_sigma=sky)
    host = c.deblend_fields(dists, measure=True)                  # the default path: stamps and catalogue on the host
    names = tuple(n[0] for n in ms.fit_flux_dtype(NB) + ms.fit_groups_dtype(NB))
    want_cols = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) +
                         DeblendFieldBatch.fit_flux_columns(NB) + DeblendFieldBatch.fit_groups_columns(NB))
    for m, (r, p, h) in enumerate(zip(res, dense, host)):
        assert r.dtype == want_cols and len(r) == len(p)
        for k in p.dtype.names:                                   # the columns of the dense fit, value for value
            if k != "shifts":
                assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].base.kind == "f"), k
        if not len(r):
            continue
        mean = np.stack([np.asarray(x) for x in h["output_images_mean"]])
        places = int((F2 - CS) / 2) + dists[m].astype(np.int64)
        want = ms.fit_fluxes_groups(mean, places, fields[m], catalogue=h, sky_sigma=sky[m], ctx=c._ctx)
        for k in names:
            assert np.array_equal(r[k], want[k], equal_nan=True), (m, k)
        g, s = go.groups(places, [0, len(places)], CS, F2)
        assert np.array_equal(r["fit_group"], g) and np.array_equal(r["fit_group_size"], s)
    cat = d.deblend_fields(dists, on_device=True, measure=True, fit_flux=True, fit_groups=True, sky_sigma=sky, return_fields=False)
    for r, q in zip(res, cat):
        for k in r.dtype.names:
            if k != "shifts":
                assert np.array_equal(r[k], q[k], equal_nan=r.dtype[k].base.kind == "f"), k
