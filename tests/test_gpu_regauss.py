"""The PSF correction on the GPU (dv_scene_regauss, dv_infer_fields_measure_psf, DeblendFieldBatch(measure=True, psf=...);
DESIGN.md section 7n) against the numpy restatement of tests/regauss_oracle.py, and the pipeline stage against the stamp-level
call, bit for bit.  The bounds are those of the specification: status equal, iterations equal or one apart, and for
converged rows the centroid to 1e-8 px, M' to 1e-8 (Mrr + Mcc) and rho4 to 1e-7; the PSF rows are held to the same.  Both
sides start from the same catalogue rows (the GPU's own measurement), so the comparison is of the correction alone."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import measure_oracle as mo
from tests import regauss_oracle as ro
from tests.test_gpu_measure import ARCH, COUNTS, CS, NB, _blob_fields, _net, _windows

pytestmark = pytest.mark.gpu

CAT = ("flux", "flux_err", "shape", "iters", "status")
RG = ("regauss", "regauss_iters", "regauss_status", "psf_shape", "psf_aux", "psf_iters", "psf_status")


def _ctx():
    from debvader_amd import engine as E

    return E.default_context()


def _double_psf(ps, seed):
    rng = np.random.default_rng(seed)
    Cc = ro.cov(rng.uniform(1.2, 1.6), rng.uniform(-0.08, 0.08), rng.uniform(-0.08, 0.08))
    op = rng.uniform(-0.5, 0.5, 2)
    return 0.85 * ro.norm_gaussian(ps, Cc, op) + 0.15 * ro.norm_gaussian(ps, 4.0 * Cc, op), Cc


def _psfs(ps):
    """K = 3: two double-Gaussian PSFs (the second not normalised) and an all-zero image, which no galaxy can use"""
    return np.stack([_double_psf(ps, 1)[0], 2.5 * _double_psf(ps, 2)[0], np.zeros((ps, ps))])


def _planes(cs, ps, full):
    """(name, plane (cs, cs), psf index): the families of the specification"""
    rng = np.random.default_rng(300 + cs)
    ctr = (cs - 1) / 2.0
    rr, cc = np.arange(cs, dtype=np.float64)[:, None], np.arange(cs, dtype=np.float64)[None, :]
    out = []
    for k in range(12 if full else 2):                       # the double-Gaussian family, seen through PSF 0 or 1
        pi = k % 2
        Cc = _double_psf(ps, 1 + pi)[1]
        Cf = ro.cov(rng.uniform(1.5, 3.0), rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4))
        og = rng.uniform(-1.0, 1.0, 2)
        out.append(("double gaussian", 0.85 * ro.norm_gaussian(cs, Cf + Cc, og, 100.0) +
                    0.15 * ro.norm_gaussian(cs, Cf + 4.0 * Cc, og, 100.0), pi))
    for k in range(12 if full else 1):                       # relu'd Gaussians with sigma = 0.02 noise
        a, b = rng.uniform(4.0, 12.0, size=2)
        M = (a, rng.uniform(-0.6, 0.6) * np.sqrt(a * b), b)
        g = mo.gaussian_stamp(cs, M, rng.uniform(-3.0, 3.0, size=2), amp=rng.uniform(0.5, 3.0))
        out.append(("noisy gaussian", np.maximum(g + rng.normal(0.0, 0.02, size=g.shape), 0.0), k % 2))
    for off in [(0.0, 0.0), (-0.7, 1.2), (2.4, -1.9)][:3 if full else 1]:
        out.append(("exponential", np.exp(-np.hypot(rr - ctr - off[0], cc - ctr - off[1]) / 2.5), 0))
    for k in range(4 if full else 0):                        # two overlapping blobs
        o1, o2 = rng.uniform(-2.0, 2.0, size=2), rng.uniform(-2.0, 2.0, size=2) + (3.0, 4.0)
        out.append(("two blobs", mo.gaussian_stamp(cs, (6.0, 0.0, 6.0), o1) + 0.6 * mo.gaussian_stamp(cs, (7.0, 1.0, 5.0), o2), 1))
    good = ro.norm_gaussian(cs, np.array([6.0, 0.5, 5.0]), (0.2, 0.3), 10.0)
    out += [("zero", np.zeros((cs, cs)), 0),                                          # status 4
            ("zero psf", good, 2), ("index -1", good, -1), ("index K", good, 3),      # status 5
            ("narrow", ro.norm_gaussian(cs, np.array([1.2, 0.0, 1.2]), (0.3, -0.2), 10.0), 0)]   # status 6
    return out


@functools.lru_cache(maxsize=None)
def _case(cs, nb, ps, full):
    """(names, stamps float32 (N, cs, cs, nb), psf_index, psf (3, ps, ps), the GPU's catalogue rows, the oracle on them):
    computed once, never written to"""
    planes = _planes(cs, ps, full)
    band = 2
    rng = np.random.default_rng(11 * cs + nb)
    stamps = np.zeros((len(planes), cs, cs, nb), np.float32)
    for i, (_, p, _) in enumerate(planes):
        for b in range(nb):
            stamps[i, :, :, b] = p if b == band else rng.uniform(0.3, 2.0) * p + rng.uniform(0.0, 0.1, size=p.shape)
    index = np.array([k for _, _, k in planes], np.int32)
    psf = _psfs(ps)
    cat = _ctx().scene_measure(stamps, band=band)
    ref = ro.regauss(stamps, cat["shape"], cat["status"], index, psf, band=band)
    for a in (stamps, index, psf) + tuple(cat.values()) + tuple(ref.values()):
        a.flags.writeable = False
    return [n for n, _, _ in planes], stamps, index, psf, cat, ref


def _compare(names, got, ref, what):
    d_it = np.abs(got["regauss_iters"].astype(int) - ref["regauss_iters"].astype(int))
    ok = ref["regauss_status"] == ro.CONVERGED
    tr = np.where(ok, ref["regauss"][:, 2] + ref["regauss"][:, 4], 1.0)
    d_c = np.abs(got["regauss"][:, :2] - ref["regauss"][:, :2]).max(axis=1)
    d_m = np.abs(got["regauss"][:, 2:5] - ref["regauss"][:, 2:5]).max(axis=1) / tr
    d_k = np.abs(got["regauss"][:, 5] - ref["regauss"][:, 5])
    print(f"{what}: status {np.bincount(ref['regauss_status'], minlength=7).tolist()}, differs on "
          f"{int((got['regauss_status'] != ref['regauss_status']).sum())} rows, iterations {ref['regauss_iters'][ok].min()} .. "
          f"{ref['regauss_iters'][ok].max()} differ by at most {d_it.max()}, centroid {d_c[ok].max():.2e} px, M' {d_m[ok].max():.2e} "
          f"of the trace, rho4 {d_k[ok].max():.2e} ({int(ok.sum())} converged of {len(ok)})")
    assert np.array_equal(got["regauss_status"], ref["regauss_status"]), list(zip(names, got["regauss_status"], ref["regauss_status"]))
    assert d_it.max() <= 1
    assert d_c[ok].max() <= 1e-8 and d_m[ok].max() <= 1e-8 and d_k[ok].max() <= 1e-7
    gone = ref["regauss_status"] >= 4
    assert np.isnan(got["regauss"][gone]).all() and (got["regauss_iters"][gone] == 0).all()
    # the PSF rows
    pk = ref["psf_status"] == ro.CONVERGED
    ptr = np.where(pk, ref["psf_shape"][:, 2] + ref["psf_shape"][:, 4], 1.0)
    assert np.array_equal(got["psf_status"], ref["psf_status"])
    assert np.abs(got["psf_iters"].astype(int) - ref["psf_iters"].astype(int)).max() <= 1
    assert np.abs(got["psf_shape"][pk, :2] - ref["psf_shape"][pk, :2]).max() <= 1e-8
    assert (np.abs(got["psf_shape"][:, 2:] - ref["psf_shape"][:, 2:]).max(axis=1) / ptr)[pk].max() <= 1e-8
    assert np.abs(got["psf_aux"][pk, 2] - ref["psf_aux"][pk, 2]).max() <= 1e-7
    assert np.allclose(got["psf_aux"][pk, :2], ref["psf_aux"][pk, :2], rtol=1e-8, atol=0.0)
    assert np.array_equal(np.isnan(got["psf_aux"]), np.isnan(ref["psf_aux"]))
    assert np.allclose(got["psf_aux"][:, 1], ref["psf_aux"][:, 1], rtol=1e-12, atol=0.0)       # FQ, a plain sum


@pytest.mark.parametrize("cs,nb,ps,full", [(31, 3, 15, True), (31, 6, 15, True), (59, 6, 21, False), (59, 6, 33, False)])
def test_scene_regauss_against_the_oracle(cs, nb, ps, full):
    names, stamps, index, psf, cat, ref = _case(cs, nb, ps, full)
    assert len(names) == (36 if full else 9)
    # the restatement alone first: the families end where the specification says
    st = dict(zip(names, ref["regauss_status"]))
    assert (st["zero"], st["zero psf"], st["index -1"], st["index K"], st["narrow"]) == (4, 5, 5, 5, 6)
    conv = {n for n, s in zip(names, ref["regauss_status"]) if s == ro.CONVERGED}
    assert conv >= ({"double gaussian", "noisy gaussian", "exponential", "two blobs"} if full else {"double gaussian", "exponential"})
    assert ref["psf_status"].tolist() == [0, 0, 3]

    got = _ctx().scene_regauss(stamps, cat["shape"], cat["status"], psf, index)
    _compare(names, got, ref, f"gpu vs oracle {cs}/{nb}/{ps}")
    # a row's result does not depend on where it sits in the batch, nor on the other bands
    perm = np.random.default_rng(1).permutation(len(names))
    shuffled = _ctx().scene_regauss(stamps[perm], cat["shape"][perm], cat["status"][perm], psf, index[perm])
    for k in RG[:3]:
        assert np.array_equal(shuffled[k], got[k][perm], equal_nan=True), k
    for k in RG[3:]:
        assert np.array_equal(shuffled[k], got[k], equal_nan=True), k
    other = np.array(stamps)
    other[..., :2] = 0.5
    o = _ctx().scene_regauss(other, cat["shape"], cat["status"], psf, index)
    assert all(np.array_equal(o[k], got[k], equal_nan=True) for k in RG)
    # one PSF for all: the rows that used PSF 1 before change, those of PSF 0 keep their bits
    one = _ctx().scene_regauss(stamps, cat["shape"], cat["status"], psf[0])
    was0 = index == 0
    assert np.array_equal(one["regauss"][was0], got["regauss"][was0], equal_nan=True) and one["psf_shape"].shape == (1, 5)
    assert np.array_equal(one["psf_shape"][0], got["psf_shape"][0])


def test_double_gaussian_family_is_corrected_on_the_gpu():
    """The figures of the specification's family (b), end to end on the GPU: measure_stamps_psf on float32 stamps"""
    from debvader_amd.measure import measurement as ms

    cases = [ro.double_gaussian_case(s) for s in range(12)]
    stamps = np.stack([c[0] for c in cases])[:, :, :, None].astype(np.float32) * np.ones(3, np.float32)
    psf = np.stack([c[1] for c in cases])
    rec = ms.measure_stamps_psf(stamps, psf, np.arange(12), ctx=_ctx())
    cat = ms.measure_stamps(stamps, ctx=_ctx())
    assert (rec["regauss_status"] == 0).all()
    for i, (_, _, Cf) in enumerate(cases):
        tr = Cf[0] + Cf[2]
        e_true, s_true = np.array([(Cf[2] - Cf[0]) / tr, 2 * Cf[1] / tr]), (Cf[0] * Cf[2] - Cf[1] ** 2) ** 0.25
        G = np.array([cat["Mrr"][i] - rec["psf_Mrr"][i], cat["Mrc"][i] - rec["psf_Mrc"][i], cat["Mcc"][i] - rec["psf_Mcc"][i]])
        e_unc, s_unc = np.array([(G[2] - G[0]) / (G[0] + G[2]), 2 * G[1] / (G[0] + G[2])]), (G[0] * G[2] - G[1] ** 2) ** 0.25
        err = (max(abs(rec["e1_corr"][i] - e_true[0]), abs(rec["e2_corr"][i] - e_true[1])), np.abs(e_unc - e_true).max(),
               abs(rec["sigma_corr"][i] / s_true - 1), abs(s_unc / s_true - 1))
        print(f"seed {i:2d}: e {err[0]:.2e} against {err[1]:.2e}, sigma {err[2]:.2e} against {err[3]:.2e}")
        assert err[0] <= 0.2 * err[1] and err[2] <= 0.2 * err[3]


def _index(n, K, seed):
    index = np.random.default_rng(seed).integers(0, K, size=n).astype(np.int32)
    index[::17] = -1
    index[5::23] = K
    return index


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_pipeline_stage_has_the_bits_of_the_stamp_level_call(dtype, monkeypatch):
    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    F = 131
    fields = _blob_fields(5, F, seed=11)
    starts, places, fp = _windows(F, COUNTS, seed=5)
    seed = 77
    psf = np.stack([_double_psf(21, 1)[0], ro.norm_gaussian(21, np.array([1.0, 0.1, 1.2]), (0.2, -0.3)), np.zeros((21, 21))])
    index = _index(len(starts), 3, seed=2)
    stamps = eng.infer_fields(fields, starts, fp, seed=seed)
    plain = eng.infer_fields_measure(fields, starts, fp, places=places, seed=seed)
    want = ctx.scene_regauss(stamps["loc"], plain["shape"], plain["status"], psf, index)
    print(f"[{dtype}] regauss_status of the {len(starts)} network stamps: {np.bincount(want['regauss_status'], minlength=7).tolist()}, "
          f"catalogue status {np.bincount(plain['status'], minlength=4).tolist()}")
    assert (want["regauss_status"][(index < 0) | (index >= 2)] >= 4).all()

    got = eng.infer_fields_measure_psf(fields, starts, fp, psf, index, places=places, seed=seed)
    assert sorted(got) == sorted(tuple(plain) + RG)
    for k in plain:                                               # every shared output has infer_fields_measure's bits
        assert np.array_equal(got[k], plain[k]), k
    for k in RG:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=True), k
    # the catalogue-only call
    only = eng.infer_fields_measure_psf(fields, starts, fp, psf, index, seed=seed, return_fields=False)
    assert sorted(only) == sorted(CAT + ("mse_center",) + RG)
    for k in only:
        assert np.array_equal(only[k], got[k], equal_nan=True), k
    # the fields uploaded in groups (see tests/test_gpu_fields_batch.py), with and without result fields
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "10")
    grouped = eng.infer_fields_measure_psf(fields, starts, fp, psf, index, places=places, seed=seed)
    for k in got:
        assert np.array_equal(grouped[k], got[k], equal_nan=True), k
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "3")
    g2 = eng.infer_fields_measure_psf(fields, starts, fp, psf, index, seed=seed, return_fields=False)
    for k in only:
        assert np.array_equal(g2[k], only[k], equal_nan=True), k
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    # other parameters reach the kernels; M = 1 is the single-field view
    b0 = eng.infer_fields_measure_psf(fields, starts, fp, psf, index, seed=seed, return_fields=False, band=0, max_iter=9,
                                      psf_sigma0=1.5)
    c0 = ctx.scene_measure(stamps["loc"], stamps["scale"], band=0, max_iter=9)
    w0 = ctx.scene_regauss(stamps["loc"], c0["shape"], c0["status"], psf, index, band=0, max_iter=9, psf_sigma0=1.5)
    assert all(np.array_equal(b0[k], w0[k], equal_nan=True) for k in RG) and b0["psf_iters"].max() <= 9
    assert np.array_equal(b0["shape"], c0["shape"]) and not np.array_equal(b0["psf_shape"], want["psf_shape"])
    s1, p1, fp1 = _windows(F, [70], seed=9)
    one = eng.infer_fields_measure_psf(fields[2:3], s1, fp1, psf[0], places=p1, seed=seed)
    ref = eng.infer_cutouts_measure_psf(fields[2], s1, psf[0], places=p1, seed=seed)
    assert "mean_field" in ref and np.array_equal(one["mean_fields"][0], ref["mean_field"])
    for k in CAT + RG:
        assert np.array_equal(one[k], ref[k], equal_nan=True), k


def test_deblend_field_batch_corrects_on_the_device():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch, batch_windows
    from debvader_amd.measure import measurement as ms

    F = 131
    fields = _blob_fields(3, F, seed=21)
    rng = np.random.default_rng(4)
    dists = [rng.integers(-30, 31, size=(n, 2)).astype(np.float64) for n in (20, 0, 45)]
    one = _double_psf(21, 1)[0]
    per_field = np.stack([one, ro.norm_gaussian(21, np.array([1.0, 0.1, 1.2]), (0.2, -0.3)), _double_psf(21, 2)[0]])

    def batch():
        net = _net("float32")                                    # the same weights ...
        net._core.seed_counter = 1234                            # ... and the same sequence of noise seeds (random per net)
        return net, DeblendFieldBatch(net, fields, CS, NB)

    plain = batch()[1].deblend_fields(dists, on_device=True, measure=True)
    starts, fp, _, _ = batch_windows(F, dists, CS)
    want_cols = np.dtype(DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB) + DeblendFieldBatch.psf_columns())
    for psf, index in ((one, np.zeros(65, np.int32)), (per_field, np.repeat([0, 1, 2], [20, 0, 45]).astype(np.int32))):
        net, a = batch()
        res = a.deblend_fields(dists, on_device=True, measure=True, psf=psf)
        eng = batch()[0]._core.engine
        out = eng.infer_fields_measure_psf(fields, starts, fp, psf, index, seed=1235, return_fields=False)
        cat = ms.psf_records(out["regauss"], out["regauss_iters"], out["regauss_status"], out["psf_shape"], out["psf_aux"], index)
        for m, (r, p) in enumerate(zip(res, plain)):
            lo, hi = int(fp[m]), int(fp[m + 1])
            assert r.dtype == want_cols and len(r) == hi - lo
            for k in p.dtype.names:                               # the columns of the same call without psf, value for value
                if k != "shifts":
                    assert np.array_equal(r[k], p[k], equal_nan=p.dtype[k].kind == "f"), k
            for k in cat.dtype.names:
                assert np.array_equal(r[k], cat[k][lo:hi], equal_nan=cat.dtype[k].kind == "f"), k
        assert np.array_equal(a.psf_moments["psf_shape"], out["psf_shape"])
        fields_a = a.get_predicted_fields()
        # return_fields=False: the same catalogue, no fields
        net, c = batch()
        only = c.deblend_fields(dists, on_device=True, measure=True, psf=psf, return_fields=False)
        for r, q in zip(res, only):
            for k in r.dtype.names:
                if k != "shifts":
                    assert np.array_equal(r[k], q[k], equal_nan=r.dtype[k].kind == "f"), k
        with pytest.raises(ValueError, match="catalogue-only"):
            c.get_predicted_fields()
        assert fields_a["predicted_mean_fields"].shape == (3, F, F, NB)


def test_refusals_come_before_any_gpu_work_and_leave_the_engine_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import Engine, _dp, _fp, _ip

    DvError, lib = _lib.DvError, _lib.lib
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    F = 131
    fields = _blob_fields(1, F, seed=11)
    starts, places, fp = _windows(F, [5], seed=5, hang=False)
    psf = np.ascontiguousarray(_psfs(21)[:2])
    index = np.array([0, 1, 0, 1, 0], np.int32)
    good = eng.infer_fields_measure_psf(fields, starts, fp, psf, index, places=places, seed=3)

    n, nb = 5, NB
    cat = [np.zeros((n, nb)), np.zeros((n, nb)), np.zeros((n, 5)), np.zeros(n, np.int32), np.zeros(n, np.int32)]
    rg = [np.zeros((n, 6)), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((2, 5)), np.zeros((2, 3)), np.zeros(2, np.int32),
          np.zeros(2, np.int32)]
    ptr = lambda a: None if a is None else (_dp(a) if a.dtype == np.float64 else _ip(a))     # noqa: E731
    f2, N, args = Engine._field_args(fields, starts, fp, places)
    mean_f, std_f, res_f = np.empty(f2.shape), np.empty(f2.shape), np.empty(f2.shape)

    def pipeline(par=None, psf_=psf, K=2, ps=21, idx=index, s0=2.0, out=None, fields_out=(None, None, None)):
        par = par or _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
        out = rg if out is None else out
        _lib.check(lib.dv_infer_fields_measure_psf(eng._h, *args, 9, C.byref(par), *fields_out, None, *map(ptr, cat), ptr(psf_), K,
                                                   ps, ptr(idx), s0, *map(ptr, out)))

    st = np.zeros((2, 31, 31, 3), np.float32)
    rows, stat, idx2 = np.zeros((2, 5)), np.zeros(2, np.int32), np.zeros(2, np.int32)
    rg2 = [np.zeros((2, 6)), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros((2, 5)), np.zeros((2, 3)), np.zeros(2, np.int32),
           np.zeros(2, np.int32)]

    def scene(x=st, psf_=psf, K=2, ps=21, band=2, s0=2.0, tol=1e-10, max_iter=200, out=None, sh=rows):
        out = rg2 if out is None else out
        _lib.check(lib.dv_scene_regauss(ctx._h, _fp(x), ptr(sh), _ip(stat), _ip(idx2), x.shape[0], x.shape[1], x.shape[3], band,
                                        ptr(psf_), K, ps, s0, tol, max_iter, *map(ptr, out)))

    for call in (pipeline, scene):
        for kw, msg in ((dict(psf_=None), "must all be given"), (dict(K=0), "at least 1"), (dict(K=-3), "at least 1"),
                        (dict(ps=4), "5 .. 33"), (dict(ps=34), "5 .. 33"), (dict(s0=0.0), "psf_sigma0"),
                        (dict(s0=float("nan")), "psf_sigma0"), (dict(s0=float("inf")), "psf_sigma0")):
            with pytest.raises(DvError, match=msg):
                call(**kw)
        for k in range(7):
            out = list(rg if call is pipeline else rg2)
            out[k] = None
            with pytest.raises(DvError, match="must all be given"):
                call(out=out)
    with pytest.raises(DvError, match="must all be given"):
        pipeline(idx=None)
    # everything dv_infer_fields_measure refuses
    for par, msg in ((_lib.DvMeasureParams(NB, 3.0, 1e-10, 200), "band"), (_lib.DvMeasureParams(2, 0.0, 1e-10, 200), "sigma0"),
                     (_lib.DvMeasureParams(2, 3.0, 0.0, 200), "tol"), (_lib.DvMeasureParams(2, 3.0, 1e-10, -1), "max_iter")):
        with pytest.raises(DvError, match=msg):
            pipeline(par=par)
    with pytest.raises(DvError, match="go together"):
        pipeline(fields_out=(_dp(mean_f), None, None))
    for kw, msg in ((dict(band=3), "band"), (dict(tol=0.0), "tol"), (dict(max_iter=-1), "max_iter"), (dict(sh=None), "must all be given"),
                    (dict(x=np.zeros((1, 65, 65, 1), np.float32), band=0), "1 .. 64 pixels")):
        with pytest.raises(DvError, match=msg):
            scene(**kw)
    # cs = 64 with ps = 33 is the largest layout the kernel takes (115 KB of LDS)
    big = np.zeros((2, 64, 64, 1), np.float32)
    big[:, :, :, 0] = ro.norm_gaussian(64, np.array([9.0, 1.0, 7.0]), (0.4, -0.6), 10.0)
    bp = np.stack([_double_psf(33, 1)[0]])
    bc = ctx.scene_measure(big, band=0)
    e = ctx.scene_regauss(big, bc["shape"], bc["status"], bp, band=0)
    w = ro.regauss(big[:1], bc["shape"][:1], bc["status"][:1], [0], bp, band=0)
    assert e["regauss_status"].tolist() == [0, 0] and np.array_equal(e["regauss"][0], e["regauss"][1])
    assert np.abs(e["regauss"][0] - w["regauss"][0]).max() < 1e-7
    # the engine completes a correct call afterwards, with the bits it gave before
    again = eng.infer_fields_measure_psf(fields, starts, fp, psf, index, places=places, seed=3)
    for k in good:
        assert np.array_equal(again[k], good[k], equal_nan=True), k
    pipeline(fields_out=(_dp(mean_f), _dp(std_f), _dp(res_f)))
    assert np.array_equal(mean_f, eng.infer_fields_composite(fields, starts, places, fp, seed=9)["mean_fields"])
    assert np.array_equal(rg[3], good["psf_shape"])
