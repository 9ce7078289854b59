"""The catalogue of the iterative many-field loop on the GPU (dv_field_set_pass_measure, dv_field_set_blend,
IterativeDeblendFieldBatch.iterative_catalogue(measure=True, blendedness=True)).  Expected values never come from the
code under test: the stacks, mse_center and field_mse from FieldSet.deblend_pass on a second set, the catalogue from
Context.scene_measure on Engine.infer_fields' stamps of the working residuals, the child sums and Bm / Bd from
Context.scene_blend - all bit for bit - and R1 / R2 from the numpy restatement of tests/blend_set_oracle.py within
1e-12 sum g |x|, respectively 1e-12 sum g x^2 (the bound tests/test_gpu_blend.py derives for sums of at most 59^2 terms in any
order plus the few ulp between two evaluations of exp; these stamps have 31^2 terms).  The sizes are those of the pipeline
tests of tests/test_gpu_blend.py: 31-pixel stamps, five 131-pixel fields of 30 / 0 / 150 / 7 / 40 stamps at max_batch = 64,
two passes, both engines, both modes."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import blend_set_oracle as bso
from tests.test_gpu_blend import COUNTS, CS, F2, NB, _blob_fields, _eq, _net, _windows

pytestmark = pytest.mark.gpu

CAT = ("flux", "flux_err", "shape", "iters", "status")
STACKS = ("work", "final", "mean", "stddev")


def _passes(eng, fields, cumulative, windows, seeds, blend=True):
    """The measured passes on a fresh set: per pass the returned dictionary and the stacks, then the end-of-loop sums."""
    fs = eng.open_field_set(fields, cumulative=cumulative)
    outs, stacks = [], []
    for (starts, places, fp), seed in zip(windows, seeds):
        outs.append(fs.deblend_pass_measure(starts, places, fp, seed=seed, blend=blend))
        stacks.append({k: fs.read(k) for k in STACKS})
    sums = fs.blend_sums() if blend else None
    fs.close()
    return outs, stacks, sums


@functools.lru_cache(maxsize=None)
def _case(dtype, mode):
    """Two measured passes and what they are compared with, computed once per engine and mode; nothing here is written to
    afterwards."""
    net = _net(dtype)                                   # max_batch = 64: chunks cross field boundaries
    eng, ctx = net._core.engine, net._core.ctx
    cumulative = mode == "cumulative"
    fields = _blob_fields(5, seed=11)
    windows = [_windows(COUNTS, seed=5 + p) for p in range(2)]     # field 1 has no stamps, field 2 has 150 > 64
    seeds = [77, 78]
    got, got_stacks, sums = _passes(eng, fields, cumulative, windows, seeds)
    plain_set = eng.open_field_set(fields, cumulative=cumulative)
    want, want_stacks, stamps, rows, child = [], [], [], [], []
    for (starts, places, fp), seed in zip(windows, seeds):
        work = plain_set.read("work")
        st = eng.infer_fields(work, starts, fp, seed=seed)
        stamps.append(st["loc"])
        rows.append(ctx.scene_measure(st["loc"], st["scale"]))
        want.append(plain_set.deblend_pass(starts, places, fp, seed=seed))
        want_stacks.append({k: plain_set.read(k) for k in STACKS})
        # W, A and npix do not read the fields: any model field serves
        child.append(ctx.scene_blend(st["loc"], rows[-1]["shape"], rows[-1]["status"], places, want_stacks[-1]["mean"],
                                     field_ptr=fp))
    plain_set.close()
    return dict(net=net, fields=fields, windows=windows, seeds=seeds, got=got, got_stacks=got_stacks, sums=sums, want=want,
                want_stacks=want_stacks, stamps=stamps, rows=rows, child=child)


@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_a_measured_pass_has_the_bits_of_the_calls_it_joins(dtype, mode):
    c = _case(dtype, mode)
    for p in range(2):
        got, want = c["got"][p], c["want"][p]
        assert sorted(got) == sorted(("mse_center", "field_mse", "child", "npix") + CAT)
        for k in STACKS:
            assert np.array_equal(c["got_stacks"][p][k], c["want_stacks"][p][k]), (p, k)
        assert _eq(got["mse_center"], want["mse_center"]) and _eq(got["field_mse"], want["field_mse"])
        assert np.isnan(got["field_mse"][1]) and not np.isnan(got["field_mse"][[0, 2, 3, 4]]).any()
        for k in CAT:
            assert _eq(got[k], c["rows"][p][k]), (p, k)
        assert got["child"].shape == (sum(COUNTS), 2) and got["npix"].dtype == np.int32
        assert _eq(got["child"], c["child"][p]["blend"][:, :2]), p
        assert _eq(got["npix"], c["child"][p]["npix"]), p
    ok = c["got"][0]["npix"] >= 0
    clipped = (c["got"][0]["npix"] > 0) & (c["got"][0]["npix"] < CS * CS)
    print(f"[{dtype} {mode}] pass 0: {int(ok.sum())} eligible of {len(ok)}, {int(clipped.sum())} clipped, "
          f"{int((c['got'][0]['npix'] == 0).sum())} wholly outside")
    assert ok.sum() >= 100 and clipped.any()
    # the second pass cut its stamps from another working residual than the first
    assert not np.array_equal(c["want_stacks"][0]["work"][0], c["fields"][0])
    # without the child sums: the same catalogue, and no resident rows are kept
    net = c["net"]
    fs = net._core.engine.open_field_set(c["fields"], cumulative=mode == "cumulative")
    bare = fs.deblend_pass_measure(*c["windows"][0], seed=c["seeds"][0], blend=False)
    assert sorted(bare) == sorted(("mse_center", "field_mse") + CAT)
    for k in bare:
        assert _eq(bare[k], c["got"][0][k]), k
    assert fs.blend_sums().shape == (0, 4)
    fs.close()


@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_end_of_loop_sums(dtype, mode):
    c = _case(dtype, mode)
    ctx = c["net"]._core.ctx
    cumulative = mode == "cumulative"
    n0 = sum(COUNTS)
    sums = c["sums"]
    assert sums.shape == (2 * n0, 4)
    stamps = np.concatenate(c["stamps"])
    shape = np.concatenate([r["shape"] for r in c["rows"]])
    status = np.concatenate([r["status"] for r in c["rows"]])
    places = np.concatenate([w[1] for w in c["windows"]])
    fps = [w[2] for w in c["windows"]]
    field = np.concatenate([np.repeat(np.arange(5), np.diff(fp)) for fp in fps])
    final_stacks = c["got_stacks"][1]
    # Bm, Bd: scene_blend on every field's rows of both passes, regrouped field by field
    order = np.concatenate([np.arange(p * n0 + fp[m], p * n0 + fp[m + 1]) for m in range(5) for p, fp in enumerate(fps)])
    fp_all = np.concatenate([[0], np.cumsum(2 * np.array(COUNTS))]).astype(np.int64)
    assert np.array_equal(field[order], np.repeat(np.arange(5), 2 * np.array(COUNTS)))
    want = ctx.scene_blend(stamps[order], shape[order], status[order], places[order], final_stacks["mean"], c["fields"],
                           field_ptr=fp_all)
    assert _eq(sums[order, 0], want["blend"][:, 2])
    if cumulative:
        assert np.isnan(sums[:, 1]).all()
    else:
        assert _eq(sums[order, 1], want["blend"][:, 3])
    # R1, R2 and the NaN pattern against the restatement
    ref = bso.sums(CS, shape, status, places, field, final_stacks["mean"], None if cumulative else c["fields"],
                   final_stacks["final"])
    assert np.array_equal(np.isnan(sums), np.isnan(ref["sums"]))
    fin = ~np.isnan(ref["sums"][:, 2])
    assert fin.sum() >= 100 and (~fin).sum() == (want["npix"] < 0).sum()
    for k in (0, 2, 3) if cumulative else (0, 1, 2, 3):
        err = np.abs(sums[fin, k] - ref["sums"][fin, k])
        scale = ref["scale"][fin, k]
        rel = err / np.where(scale > 0, scale, 1.0)
        print(f"[{dtype} {mode}] {'Bm Bd R1 R2'.split()[k]}: worst error {rel.max():.2e} of its scale (bound 1e-12), "
              f"{int((scale == 0).sum())} rows wholly outside")
        assert (err <= 1e-12 * scale).all(), k
    # the residual is not vacuous: a second moment well above rounding on most rows
    assert (sums[fin, 3] > 0).sum() >= fin.sum() // 2


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_rerun_and_independence_of_the_other_fields(dtype):
    c = _case(dtype, "reference")
    eng = c["net"]._core.engine
    again, _, sums2 = _passes(eng, c["fields"], False, c["windows"], c["seeds"])
    for p in range(2):
        for k in again[p]:
            assert again[p][k].tobytes() == c["got"][p][k].tobytes(), (p, k)
    assert sums2.tobytes() == c["sums"].tobytes()
    # field 0 stays first (its noise rows do not move); the others are replaced, and there are fewer of them
    counts = [30, 70, 0, 5]
    others = _blob_fields(4, seed=99)
    others[0] = c["fields"][0]
    windows = []
    for p in range(2):
        st, pl, fp = _windows(counts, seed=31 + p)
        st[:30], pl[:30] = c["windows"][p][0][:30], c["windows"][p][1][:30]
        windows.append((st, pl, fp))
    moved, stacks, sums3 = _passes(eng, others, False, windows, c["seeds"])
    n0, n1 = sum(COUNTS), sum(counts)
    for p in range(2):
        for k in CAT + ("mse_center", "child", "npix"):
            assert moved[p][k][:30].tobytes() == c["got"][p][k][:30].tobytes(), (p, k)
        assert moved[p]["field_mse"][0] == c["got"][p]["field_mse"][0]
        assert np.array_equal(stacks[p]["final"][0], c["got_stacks"][p]["final"][0])
        assert sums3[p * n1:p * n1 + 30].tobytes() == c["sums"][p * n0:p * n0 + 30].tobytes(), p
    assert not np.array_equal(moved[0]["flux"][30:60], c["got"][0]["flux"][30:60])


def _loop_net(dtype):
    """Freshly initialised weights predict stamps that are nearly zero; a bias of 1 on the head's mean channels makes every
    stamp remove about one unit of flux per pixel, so that the passes differ (tests/test_gpu_iterative_batch.py)."""
    net = _net(dtype)
    eng = net._core.engine
    bias = eng.get_param("dec/head/bias")
    bias[:NB] = 1.0
    eng.set_param("dec/head/bias", bias)
    return net


@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_the_class_with_and_without_the_catalogue(dtype, mode):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch as B
    from debvader_amd.measure.measurement import blend_dtype, catalogue_dtype, residual_dtype

    fields = np.concatenate([_blob_fields(3, seed=41), np.random.default_rng(46).normal(0, 0.05, size=(1, F2, F2, NB))])

    def run(**kw):
        net = _loop_net(dtype)                                   # the same weights and the same sequence of noise seeds
        net._core.seed_counter = 500
        it = B(net, fields, CS, NB)
        res = (it.iterative_catalogue if kw else it.iterative_deblending)(mode=mode, max_iterations=3 if mode == "cumulative" else None, **kw)
        return it, res, net._core.seed_counter

    plain, res0, seeds0 = run()
    full, res1, seeds1 = run(measure=True, blendedness=True)
    lean, res2, seeds2 = run(measure=True, blendedness=True, return_fields=False)
    assert seeds0 == seeds1 == seeds2 > 500
    passes = [len(m) for m in plain.mse]
    print(f"[{dtype} {mode}] passes per field {passes}, galaxies per field {[len(r) for r in res0]}, rows seen before "
          f"{[int((r['seen_before'] >= 0).sum()) for r in res1]}, eligible {[int((r['blend_npix'] >= 0).sum()) for r in res1]}")
    assert max(passes) >= 2 and sum(len(r) for r in res0) >= 10
    assert full.mse == plain.mse == lean.mse
    assert np.array_equal(full.get_residual_fields(), plain.get_residual_fields())
    for k, v in plain.get_predicted_fields().items():
        assert np.array_equal(full.get_predicted_fields()[k], v), k
    with pytest.raises(ValueError, match="return_fields"):
        lean.get_residual_fields()
    want = np.dtype(B.COLUMNS + catalogue_dtype(NB) + [("seen_before", "<i8")] + blend_dtype() + residual_dtype())
    for m, (p, r, q) in enumerate(zip(res0, res1, res2)):
        assert r.dtype == want and q.dtype == want and len(p) == len(r) == len(q)
        for k in p.dtype.names:                                  # the shared columns
            if k == "shifts":
                assert all(np.array_equal(x, y) for x, y in zip(r[k], p[k]))
            else:
                assert _eq(np.asarray(r[k]), np.asarray(p[k])), (m, k)
        for k in r.dtype.names:                                  # the same catalogue without the fields
            if k != "shifts":
                assert _eq(np.asarray(r[k]), np.asarray(q[k])), (m, k)
        assert (r["seen_before"][r["iteration"] == 0] == -1).all() and (r["seen_before"] < np.arange(len(r))).all()
        if mode == "cumulative":
            assert np.isnan(r["blend_data"]).all() and np.isnan(r["blendedness_data"]).all()
        ok = r["blend_npix"] > 0
        assert np.isfinite(r["resid_rms"][ok]).all() and (r["resid_rms"][ok] >= 0).all()
        assert np.isnan(r["resid_mean"][r["blend_npix"] < 0]).all()
    # the inputs are not vacuous: galaxies that were measured, and rows of later passes that stand on earlier ones
    assert sum(int((r["blend_npix"] > 0).sum()) for r in res1) >= 5
    assert any((r["seen_before"] >= 0).any() for r in res1)


def test_refusals_come_before_any_gpu_work_and_leave_the_set_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import _dp, _ip
    from debvader_amd.model import model

    DvError, lib = _lib.DvError, _lib.lib
    c = _case("float32", "reference")
    eng = c["net"]._core.engine
    fields = c["fields"]
    starts, places, fp = c["windows"][0]
    n = len(starts)
    fs = eng.open_field_set(fields)
    first = fs.deblend_pass_measure(starts, places, fp, seed=77)
    for k in first:
        assert _eq(first[k], c["got"][0][k]), k
    before = {k: fs.read(k) for k in STACKS}
    i64 = C.POINTER(C.c_int64)
    mc, fm = np.zeros(n), np.zeros(5)
    flux, ferr, shape = np.zeros((n, NB)), np.zeros((n, NB)), np.zeros((n, 5))
    iters, status, child, npix = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2)), np.zeros(n, np.int32)
    sums = np.zeros((n, 4))

    def raw_pass(par, st=starts, child_=child, npix_=npix, h=None):
        return lib.dv_field_set_pass_measure(h or fs._h, _ip(st), _ip(places), fp.ctypes.data_as(i64), n, 77,
                                             C.byref(par) if par is not None else None, _dp(mc), _dp(fm), _dp(flux), _dp(ferr),
                                             _dp(shape), _ip(iters), _ip(status), _dp(child_), None if npix_ is None else _ip(npix_))

    good = _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
    # the end-of-loop call: a wrong row count, a band outside the fields'
    assert lib.dv_field_set_blend(fs._h, 2, n + 1, _dp(sums)) == -1 and "resident rows" in _lib.last_error()
    assert lib.dv_field_set_blend(fs._h, 2, 0, _dp(sums)) == -1
    assert lib.dv_field_set_blend(fs._h, NB, n, _dp(sums)) == -1 and "band" in _lib.last_error()
    with pytest.raises(ValueError, match="band"):
        fs.blend_sums(band=NB)
    # the pass: what dv_infer_fields_measure refuses, what dv_field_set_pass refuses, half a pair of child outputs
    assert raw_pass(_lib.DvMeasureParams(NB, 3.0, 1e-10, 200)) == -1 and "band" in _lib.last_error()
    assert raw_pass(_lib.DvMeasureParams(2, 0.0, 1e-10, 200)) == -1 and "sigma0" in _lib.last_error()
    assert raw_pass(None) == -1
    assert raw_pass(good, npix_=None) == -1 and "go together" in _lib.last_error()
    bad = starts.copy()
    bad[3] = (F2 - CS + 1, 0)
    assert raw_pass(good, st=bad) == -1 and "leaves the 131-pixel field" in _lib.last_error()
    with pytest.raises(DvError, match="leaves the 131-pixel field"):
        fs.deblend_pass_measure(bad, places, fp, seed=77)
    with pytest.raises(ValueError, match="band"):
        fs.deblend_pass_measure(starts, places, fp, seed=77, band=NB)
    # nothing moved: the stacks are what they were, and the set still holds the rows of its one pass - no more, no fewer
    for k in STACKS:
        assert np.array_equal(fs.read(k), before[k]), k
    assert lib.dv_field_set_blend(fs._h, 2, n, _dp(sums)) == 0
    second = fs.deblend_pass_measure(*c["windows"][1], seed=78)
    for k in second:
        assert _eq(second[k], c["got"][1][k]), k
    assert _eq(fs.blend_sums(), c["sums"])
    # a configuration of 91-pixel stamps: refused by the binding and by the library, and its set stays usable
    big, _, _, _ = model.create_model_vae(input_shape=(91, 91, 3), latent_dim=8, filters=[8, 16], kernels=[3, 3], max_batch=4,
                                          seed=3, dtype="float32")
    f91 = np.random.default_rng(0).normal(0, 0.05, size=(1, 100, 100, 3))
    fs91 = big._core.engine.open_field_set(f91)
    s91, fp91 = np.array([[4, 5]], np.int32), np.array([0, 1], np.int64)
    with pytest.raises(ValueError, match="at most 90"):
        fs91.deblend_pass_measure(s91, s91, fp91, seed=1)
    par3 = _lib.DvMeasureParams(2, 3.0, 1e-10, 200)
    o = [np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 5))]
    assert lib.dv_field_set_pass_measure(fs91._h, _ip(s91), _ip(s91), fp91.ctypes.data_as(i64), 1, 1, C.byref(par3), _dp(mc),
                                         _dp(fm), _dp(o[0]), _dp(o[1]), _dp(o[2]), _ip(iters), _ip(status), _dp(child),
                                         _ip(npix)) == -1
    assert "at most 90 pixels" in _lib.last_error()
    assert np.array_equal(fs91.read("work"), f91) and fs91.blend_sums().shape == (0, 4)
    fs91.close()
    # a closed set: the binding and the library both refuse
    raw = C.c_void_p(fs._h.value)
    fs.close()
    with pytest.raises(DvError, match="closed"):
        fs.blend_sums()
    with pytest.raises(DvError, match="closed"):
        fs.deblend_pass_measure(starts, places, fp, seed=77)
    assert lib.dv_field_set_blend(raw, 2, 2 * n, _dp(np.zeros((2 * n, 4)))) == -5
    assert raw_pass(good, h=raw) == -5
    # afterwards a fresh set gives the expected bits
    again, _, sums2 = _passes(eng, fields, False, c["windows"], c["seeds"])
    assert all(_eq(again[1][k], c["got"][1][k]) for k in again[1]) and _eq(sums2, c["sums"])
