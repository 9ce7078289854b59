"""The joint flux fit of all passes of the iterative many-field loop on the GPU (dv_field_set_keep_stamps,
dv_field_set_fit_flux, IterativeDeblendFieldBatch.iterative_catalogue(fit_flux=True)).  Expected values
never come from the code under test: the stand-alone calls Context.scene_fit_flux, scene_fit_flux_sky and
scene_fit_flux_nonneg get the mean stamps Engine.infer_fields returns for every pass's working residual, regrouped field by
field by the index arithmetic of this file (the `order` of tests/test_gpu_iterative_catalogue.py), and the uploaded fields as
the data.  Every comparison is bit for bit: the kernels that do the arithmetic are the stand-alone ones in the same order, and
the regrouping is a copy.  The sizes are those of tests/test_gpu_iterative_catalogue.py: 31-pixel stamps, five 131-pixel
fields of 30 / 0 / 150 / 7 / 40 stamps per pass at max_batch = 64, two passes, both engines, both modes - field 2 has 300
unknowns, more than a workgroup has threads and more than one chunk per pass; field 3's second pass repeats the windows of
its first, so its system holds near-duplicates."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_gpu_blend import COUNTS, CS, F2, NB, _blob_fields, _eq, _net, _windows
from tests.test_gpu_iterative_catalogue import STACKS, _loop_net, _passes
from tests.test_gpu_iterative_catalogue import _case as _catalogue_case

pytestmark = pytest.mark.gpu

M = 5
ROW_KEYS = ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status", "fit_chi2", "fit_npix", "fit_scale_free",
            "fit_clamped", "fit_dual")
# (name, sky_order, weighted, nonneg)
VARIANTS = [("plain", None, False, False), ("weighted", None, True, False), ("sky0", 0, False, False), ("sky1", 1, False, False),
            ("sky1 weighted", 1, True, False), ("nonneg", None, False, True), ("nonneg sky0 weighted", 0, True, True)]


def _two_pass_windows():
    """The windows of tests/test_gpu_iterative_catalogue.py, with field 3's second pass repeating its first"""
    windows = [_windows(COUNTS, seed=5 + p) for p in range(2)]
    lo, hi = int(windows[0][2][3]), int(windows[0][2][4])
    windows[1][0][lo:hi], windows[1][1][lo:hi] = windows[0][0][lo:hi], windows[0][1][lo:hi]
    return windows


def _order(fps):
    """order[dst] = resident row, field by field, pass after pass inside a field; and the joint field_ptr"""
    n0 = np.concatenate([[0], np.cumsum([int(fp[-1]) for fp in fps])])
    order = np.concatenate([np.arange(n0[p] + fp[m], n0[p] + fp[m + 1]) for m in range(M) for p, fp in enumerate(fps)])
    counts = np.sum([np.diff(fp) for fp in fps], axis=0)
    return order.astype(np.int64), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _measured_set(eng, fields, cumulative, windows, seeds, keep=True):
    """A set with the passes measured (stamps kept) and, read before every pass, the working residual the pass cut from"""
    fs = eng.open_field_set(fields, cumulative=cumulative)
    if keep:
        fs.keep_stamps()
    outs, stacks, works = [], [], []
    for (starts, places, fp), seed in zip(windows, seeds):
        works.append(fs.read("work"))
        outs.append(fs.deblend_pass_measure(starts, places, fp, seed=seed))
        stacks.append({k: fs.read(k) for k in STACKS})
    return fs, outs, stacks, works


def _stamps(eng, works, windows, seeds):
    return np.concatenate([eng.infer_fields(w, st, fp, seed=seed)["loc"] for w, (st, _, fp), seed in zip(works, windows, seeds)])


def _weights_and_data(fields):
    """Random positive weights with some zeros, and the fields with one NaN pixel under a zero weight"""
    rng = np.random.default_rng(8)
    W = rng.uniform(0.5, 2.0, size=fields.shape)
    W[rng.random(fields.shape) < 0.1] = 0.0
    data = fields.copy()
    W[2, 60, 61, :] = 0.0
    data[2, 60, 61, 2] = np.nan
    return W, data


@functools.lru_cache(maxsize=None)
def _case(dtype, mode):
    """Two measured passes with the stamps kept - the set stays open - and what the fit is compared with; nothing here is
    written to afterwards."""
    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    cumulative = mode == "cumulative"
    fields = _blob_fields(M, seed=11)
    windows = _two_pass_windows()
    seeds = [77, 78]
    fs, outs, stacks, works = _measured_set(eng, fields, cumulative, windows, seeds)
    stamps = _stamps(eng, works, windows, seeds)
    places = np.concatenate([w[1] for w in windows])
    order, fp_all = _order([w[2] for w in windows])
    W, data = _weights_and_data(fields)
    return dict(net=net, eng=eng, ctx=ctx, fs=fs, fields=fields, windows=windows, seeds=seeds, outs=outs, stacks=stacks,
                stamps=stamps[order], places=places[order], order=order, fp_all=fp_all, W=W, data=data, cumulative=cumulative)


def _standalone(ctx, stamps, places, data, fp_all, sky, W, nonneg, **kw):
    if nonneg:
        return ctx.scene_fit_flux_nonneg(stamps, places, data, field_ptr=fp_all, sky_order=sky, weight_fields=W, **kw)
    if sky is not None:
        return ctx.scene_fit_flux_sky(stamps, places, data, field_ptr=fp_all, sky_order=sky, weight_fields=W, **kw)
    return ctx.scene_fit_flux(stamps, places, data, field_ptr=fp_all, weight_fields=W, **kw)


def _same(got, want, order, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        a = got[k][order] if k in ROW_KEYS else got[k]
        assert _eq(a, want[k]), (what, k)


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_the_joint_fit_has_the_bits_of_the_standalone_calls(dtype, mode, variant):
    name, sky, weighted, nonneg = variant
    c = _case(dtype, mode)
    assert np.diff(c["fp_all"]).tolist() == [60, 0, 300, 14, 80]
    W = c["W"] if weighted else None
    data = c["data"] if weighted else c["fields"]                   # (the NaN pixel needs its zero weight)
    want = _standalone(c["ctx"], c["stamps"], c["places"], data, c["fp_all"], sky, W, nonneg)
    got = c["fs"].fit_flux(data_fields=data, weight_fields=W, sky_order=sky, nonneg=nonneg)
    _same(got, want, c["order"], name)
    assert got["fit_scale"].shape == (2 * sum(COUNTS), NB)
    st = got["fit_status"]
    print(f"[{dtype} {mode} {name}] status 0 / 4 / 5: {int((st == 0).sum())} / {int((st == 4).sum())} / {int((st == 5).sum())} of "
          f"{st.size} (row, band) pairs" + (f", clamped {int(got['fit_clamped'].sum())}" if nonneg else ""))
    assert (st == 0).sum() >= st.size // 2                         # the system is not vacuous
    if not weighted and not c["cumulative"]:                       # the resident base is the uploaded fields
        _same(c["fs"].fit_flux(sky_order=sky, nonneg=nonneg), want, c["order"], name + " (resident base)")


@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_the_switch_changes_no_bit_of_the_passes(dtype, mode):
    """Off: tests/test_gpu_iterative_catalogue.py compares the passes with the calls they join.  On: every output of every pass,
    every stack and the end-of-loop sums have the bits of the passes without it."""
    off = _catalogue_case(dtype, mode)
    eng = off["net"]._core.engine
    fs, outs, stacks, _ = _measured_set(eng, off["fields"], mode == "cumulative", off["windows"], off["seeds"])
    sums = fs.blend_sums()
    fs.close()
    for p in range(2):
        assert sorted(outs[p]) == sorted(off["got"][p])
        for k in outs[p]:
            assert _eq(outs[p][k], off["got"][p][k]), (p, k)
        for k in STACKS:
            assert np.array_equal(stacks[p][k], off["got_stacks"][p][k]), (p, k)
    assert _eq(sums, off["sums"])
    again, _, sums2 = _passes(eng, off["fields"], mode == "cumulative", off["windows"], off["seeds"])
    assert all(_eq(again[p][k], off["got"][p][k]) for p in range(2) for k in again[p]) and _eq(sums2, off["sums"])


def test_the_stamp_store_grows_with_the_rows():
    """227 + 227 + 600 rows cross the first capacity of 1024: the stamps of the first two passes are copied over"""
    c = _case("float32", "reference")
    eng, ctx = c["eng"], c["ctx"]
    windows = c["windows"] + [_windows([250, 0, 150, 100, 100], seed=19)]
    seeds = c["seeds"] + [79]
    fs, outs, _, works = _measured_set(eng, c["fields"], False, windows, seeds)
    stamps = _stamps(eng, works, windows, seeds)
    order, fp_all = _order([w[2] for w in windows])
    assert len(order) == 1054 and np.diff(fp_all).tolist() == [310, 0, 450, 114, 180]
    places = np.concatenate([w[1] for w in windows])
    want = ctx.scene_fit_flux(stamps[order], places[order], c["fields"], field_ptr=fp_all)
    _same(fs.fit_flux(), want, order, "three passes")
    fs.close()
    # the first two passes are those of the shared case
    for p in range(2):
        assert all(_eq(outs[p][k], c["outs"][p][k]) for k in outs[p])


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_rerun_independence_and_sub_ranges(dtype):
    c = _case(dtype, "reference")
    fs, eng = c["fs"], c["eng"]
    first = fs.fit_flux(sky_order=1, nonneg=True)
    again = fs.fit_flux(sky_order=1, nonneg=True)
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)
    # the scratch of field 2 alone, NB x 300 x 300 doubles: fields {0, 1}, {2}, {3, 4} go through it one after the other
    plain = fs.fit_flux()
    need = NB * 300 * 300 * 8
    split = fs.fit_flux(scratch_bytes=need)
    assert all(plain[k].tobytes() == split[k].tobytes() for k in plain)
    # a pivot bound at which rows are dropped (none is at the default, not even in the repeated windows of field 3)
    loose = fs.fit_flux(min_pivot=0.3)
    _same(loose, c["ctx"].scene_fit_flux(c["stamps"], c["places"], c["fields"], field_ptr=c["fp_all"], min_pivot=0.3), c["order"],
          "min_pivot 0.3")
    print(f"[{dtype}] min_pivot 0.3: {int((loose['fit_status'] == 5).sum())} (row, band) pairs dropped, "
          f"{int((loose['fit_status'][:sum(COUNTS)] == 5).sum())} of them in pass 0")
    # field 0 stays first; the others are replaced, and there are fewer of them
    counts = [30, 70, 0, 5]
    others = _blob_fields(4, seed=99)
    others[0] = c["fields"][0]
    windows = []
    for p in range(2):
        st, pl, fp = _windows(counts, seed=31 + p)
        st[:30], pl[:30] = c["windows"][p][0][:30], c["windows"][p][1][:30]
        windows.append((st, pl, fp))
    fs2, _, _, _ = _measured_set(eng, others, False, windows, c["seeds"])
    moved = fs2.fit_flux(sky_order=1, nonneg=True)
    fs2.close()
    n0, n1 = sum(COUNTS), sum(counts)
    for k in ROW_KEYS:
        if k in first:
            for p in range(2):
                assert moved[k][p * n1:p * n1 + 30].tobytes() == first[k][p * n0:p * n0 + 30].tobytes(), (k, p)
    for k in ("sky_coef", "sky_cov", "sky_status", "sky_npix", "nonneg_iters", "nonneg_status"):
        assert moved[k][0].tobytes() == first[k][0].tobytes(), k


def test_refusals_come_before_any_gpu_work_and_leave_the_set_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import _dp, _ip

    DvError, lib = _lib.DvError, _lib.lib
    c = _case("float32", "reference")
    fs, eng, fields = c["fs"], c["eng"], c["fields"]
    n = 2 * sum(COUNTS)
    want = fs.fit_flux()
    before = {k: fs.read(k) for k in STACKS}
    sums = fs.blend_sums()
    o = [np.zeros((n, NB)) for _ in range(4)] + [np.zeros((n, NB), np.int32)]
    par = _lib.DvFitFluxParams(1e-8, 256 << 20)
    nulls = [None] * 11

    def raw(h=None, rows=n, data=None, sky=-1, par_=par, outs=None):
        ptrs = [_dp(a) for a in o[:4]] + [_ip(o[4])] if outs is None else outs
        return lib.dv_field_set_fit_flux(h or fs._h, rows, data, None, sky, 0, C.byref(par_), 1, *ptrs, *nulls)

    assert raw() == 0 and all(_eq(a, want[k]) for a, k in zip(o, ROW_KEYS))
    assert raw(rows=n + 1) == -1 and "resident rows" in _lib.last_error()
    assert raw(sky=2) == -1 and "sky_order" in _lib.last_error()
    assert raw(sky=0) == -1 and "sky_coef" in _lib.last_error()              # the sky outputs are missing
    assert raw(par_=_lib.DvFitFluxParams(1.5, 256 << 20)) == -1 and "min_pivot" in _lib.last_error()
    assert raw(par_=_lib.DvFitFluxParams(1e-8, 0)) == -1 and "scratch_bytes" in _lib.last_error()
    assert raw(par_=_lib.DvFitFluxParams(1e-8, NB * 300 * 300 * 8 - 1)) == -1
    assert "field 2 has 300 galaxies" in _lib.last_error() and "scratch" in _lib.last_error()
    assert lib.dv_field_set_fit_flux(fs._h, n, None, None, -1, 0, C.byref(par), 1, *[_dp(a) for a in o[:4]], _ip(o[4]),
                                     _dp(o[0]), *nulls[1:]) == -1 and "fit_chi2" in _lib.last_error()
    assert lib.dv_field_set_keep_stamps(fs._h, 0) == -5 and "resident rows" in _lib.last_error()
    with pytest.raises(DvError, match="resident rows"):
        fs.keep_stamps()
    for bad in (dict(sky_order=2), dict(min_pivot=0.0), dict(scratch_bytes=0), dict(nonneg=True, max_iter=0),
                dict(data_fields=fields[:, :-1]), dict(weight_fields=fields[:2])):
        with pytest.raises(ValueError):
            fs.fit_flux(**bad)
    # a set that never kept its stamps, and NULL data on a cumulative set
    bare = eng.open_field_set(fields)
    bare.deblend_pass_measure(*c["windows"][0], seed=77)
    with pytest.raises(DvError, match="keeps no stamps"):
        bare.fit_flux()
    assert bare.blend_sums().shape == (n // 2, 4)                               # (the set still answers)
    bare.close()
    cum = _case("float32", "cumulative")
    with pytest.raises(ValueError, match="cumulative"):
        cum["fs"].fit_flux()
    assert raw(h=cum["fs"]._h) == -1 and "cumulative" in _lib.last_error()
    # a field of 600 + 600 stamps over two passes: refused with the field's index and the count
    crowd = eng.open_field_set(fields[:2])
    crowd.keep_stamps()
    for p in range(2):
        st, pl, fp = _windows([3, 600], seed=50 + p)
        crowd.deblend_pass_measure(st, pl, fp, seed=90 + p)
    with pytest.raises(DvError, match="field 1 has 1200 galaxies"):
        crowd.fit_flux()
    assert crowd.blend_sums().shape == (1206, 4)
    crowd.close()
    # nothing moved: the stacks, the rows and the fit are what they were
    for k in STACKS:
        assert np.array_equal(fs.read(k), before[k]), k
    assert _eq(fs.blend_sums(), sums)
    after = fs.fit_flux()
    assert all(after[k].tobytes() == want[k].tobytes() for k in want)
    # a closed set: the binding and the library both refuse
    gone = eng.open_field_set(fields[:1])
    handle = C.c_void_p(gone._h.value)
    gone.close()
    with pytest.raises(DvError, match="closed"):
        gone.fit_flux()
    with pytest.raises(DvError, match="closed"):
        gone.keep_stamps()
    assert lib.dv_field_set_keep_stamps(handle, 1) == -5
    assert raw(h=handle, rows=0) == -5


@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_the_class_with_and_without_the_fit(dtype, mode):
    from debvader_amd.deblend.field_deblender import batch_windows
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch as B
    from debvader_amd.measure import measurement as ms

    fields = np.concatenate([_blob_fields(3, seed=41), np.random.default_rng(46).normal(0, 0.05, size=(1, F2, F2, NB))])
    rng = np.random.default_rng(3)
    W = rng.uniform(0.5, 2.0, size=fields.shape)
    W[rng.random(fields.shape) < 0.1] = 0.0
    cumulative = mode == "cumulative"

    def run(**kw):
        net = _loop_net(dtype)                                   # the same weights and the same sequence of noise seeds
        net._core.seed_counter = 500
        it = B(net, fields, CS, NB)
        res = it.iterative_catalogue(mode=mode, max_iterations=3 if cumulative else None, measure=True, **kw)
        return it, res, net

    plain, res0, _ = run(blendedness=True)
    sky = np.linspace(0.04, 0.06, NB)
    fit, res1, net = run(blendedness=True, fit_flux=True, sky_sigma=sky)
    full, res2, _ = run(fit_flux=True, fit_weights=W, fit_sky=1, fit_nonneg=True, return_fields=False)
    assert fit.mse == plain.mse == full.mse and max(len(m) for m in plain.mse) >= 2
    assert np.array_equal(fit.get_residual_fields(), plain.get_residual_fields())
    for k, v in plain.get_predicted_fields().items():
        assert np.array_equal(fit.get_predicted_fields()[k], v), k
    assert fit.sky_fit is None and fit.nonneg_fit is None
    assert full.sky_fit["sky_coef"].shape == (4, NB, 3) and full.nonneg_fit["nonneg_iters"].shape == (4, NB)
    base = B.COLUMNS + B.catalogue_columns(NB, True)
    assert all(r.dtype == np.dtype(base + ms.fit_flux_dtype(NB)) for r in res1)
    lean = B.COLUMNS + B.catalogue_columns(NB, False)
    assert all(r.dtype == np.dtype(lean + ms.fit_flux_weighted_dtype(NB) + ms.fit_sky_dtype(NB) + ms.fit_nonneg_dtype(NB))
               for r in res2)
    # the stamps of every pass, re-derived: a plain set walks the same passes, infer_fields cuts from its working residual
    eng, ctx = net._core.engine, net._core.ctx
    for m in range(4):
        for k in res0[m].dtype.names:                            # every column shared with the run without the fit
            if k == "shifts":
                continue
            assert _eq(np.asarray(res1[m][k]), np.asarray(res0[m][k])), (m, k)
            if k in res2[m].dtype.names:
                assert _eq(np.asarray(res2[m][k]), np.asarray(res0[m][k])), (m, k)
    passes = max(len(mm) for mm in plain.mse)
    po = int((F2 - CS) / 2)
    ref = eng.open_field_set(fields, cumulative=cumulative)
    stamps, places = [[] for _ in range(4)], [[] for _ in range(4)]
    eng.set_normalise(False)
    for k in range(passes):
        rows = [r[r["iteration"] == k] for r in res0]
        st, fp, _, dd = batch_windows(F2, [np.stack([r["galaxy_distances_to_center_x"], r["galaxy_distances_to_center_y"]], axis=1)
                                           for r in rows], CS)
        assert np.diff(fp).tolist() == [len(r) for r in rows]
        pl = (po + dd).astype(np.int64)
        seed = 501 + k
        work = ref.read("work")
        loc = eng.infer_fields(work, st, fp, seed=seed)["loc"]
        out = ref.deblend_pass(st, pl, fp, seed=seed)
        for m in range(4):
            assert _eq(out["mse_center"][fp[m]:fp[m + 1]], np.asarray(rows[m]["mse_center"])), (k, m)   # the same windows
            stamps[m].append(loc[fp[m]:fp[m + 1]])
            places[m].append(pl[fp[m]:fp[m + 1]])
    ref.close()
    dropped = 0
    for m in range(4):
        if not len(res0[m]):
            assert len(res1[m]) == 0 and len(res2[m]) == 0
            continue
        s, p = np.concatenate(stamps[m]), np.concatenate(places[m])
        want = ms.fit_fluxes(s, p, fields[m], catalogue=res0[m], sky_sigma=sky)
        for k in want.dtype.names:
            assert _eq(np.asarray(res1[m][k]), np.asarray(want[k])), (m, k)
        want2, per_field = ms.fit_fluxes_nonneg(s, p, fields[m], sky_order=1, weight_fields=W[m], catalogue=res0[m])
        for k in want2.dtype.names:
            assert _eq(np.asarray(res2[m][k]), np.asarray(want2[k])), (m, k)
        for k, v in per_field.items():
            got = (full.sky_fit if k.startswith("sky") else full.nonneg_fit)[k]
            assert _eq(got[m:m + 1], v), (m, k)
        dropped += int((res1[m]["fit_status"] == 5).sum())
    print(f"[{dtype} {mode}] passes per field {[len(mm) for mm in plain.mse]}, galaxies {[len(r) for r in res0]}, "
          f"(row, band) pairs dropped as copies of earlier ones: {dropped}")
    assert sum(len(r) for r in res0) >= 10
