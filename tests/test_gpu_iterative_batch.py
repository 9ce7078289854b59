"""The resident field set (dv_field_set_*, engine.FieldSet) and IterativeDeblendFieldBatch against the entry points they
replace.  Expected values come only from calls that exist without the set and are promised
bit-identical to each other - Engine.infer_fields / infer_fields_composite, Context.scene_composite in object order,
Context.scene_detect, detect_objects_batch, metrics.mse - never from the code under test.  Everything is compared bit for
bit except field_mse, which has a summation order of its own: both it and metrics.mse are sums of n = F * F * bands
non-negative float64 terms, any summation order of which lies within (n - 1) * 2^-53 relative of the exact sum, so the two
differ by at most 2 * n * 2^-53 relative (the squares themselves are the same roundings on both sides)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_fields_batch import COUNTS, CS, NB, _blob_fields, _case, _net

pytestmark = pytest.mark.gpu


def _mse_close(got, exp, n):
    print(f"field_mse {got!r} metrics.mse {exp!r} rel {abs(got - exp) / exp if exp else 0.0:.3e} bound {2 * n * 2.0 ** -53:.3e}")
    return abs(got - exp) <= 2 * n * 2.0 ** -53 * abs(exp)


def _composited(ctx, start, stamps32, dist, sign):
    return ctx.scene_composite(start, stamps32.astype(np.float64), dist, sign)


def _expected_pass(net, state, starts, places, fp, seed, cumulative):
    """One pass restated: eng.infer_fields on the working residuals, then ctx.scene_composite per field in object order."""
    ctx, eng = net._core.ctx, net._core.engine
    F = state["base"].shape[1]
    po = int((F - CS) / 2)
    exp = eng.infer_fields(state["work"], starts, fp, seed=seed)
    new = {k: v.copy() for k, v in state.items()}
    for m in range(len(state["base"])):
        lo, hi = int(fp[m]), int(fp[m + 1])
        if hi == lo:
            continue
        dist = (places[lo:hi] - po).astype(np.float64)
        new["work"][m] = _composited(ctx, state["work" if cumulative else "base"][m], exp["loc"][lo:hi], dist, -1.0)
        new["final"][m] = _composited(ctx, state["final"][m], exp["loc"][lo:hi], dist, -1.0)
        new["mean"][m] = _composited(ctx, state["mean"][m], exp["loc"][lo:hi], dist, 1.0)
        new["stddev"][m] = _composited(ctx, state["stddev"][m], exp["scale"][lo:hi], dist, 1.0)
    return new


def _initial(fields):
    return {"base": fields.copy(), "work": fields.copy(), "final": fields.copy(), "mean": np.zeros_like(fields),
            "stddev": np.zeros_like(fields)}


@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_a_pass_equals_the_composition_it_replaces(dtype, mode):
    from debvader_amd.training.metrics import mse

    net = _net(dtype)                                   # max_batch = 64: chunks cross field boundaries
    eng = net._core.engine
    F = 131
    fields = _blob_fields(5, F, seed=11)
    cumulative = mode == "cumulative"
    state = _initial(fields)
    fs = eng.open_field_set(fields, cumulative=cumulative)
    for p in range(2):
        starts, places, fp = _case(F, COUNTS, seed=5 + p)         # field 1 has no stamps, field 2 has 150 > 64
        seed = 77 + p
        new = _expected_pass(net, state, starts, places, fp, seed, cumulative)
        ref_mse_center = eng.infer_fields_composite(state["work"], starts, places, fp, seed=seed)["mse_center"]
        out = fs.deblend_pass(starts, places, fp, seed=seed)
        for k in ("work", "final", "mean", "stddev"):
            got = fs.read(k)
            for m in range(5):
                assert np.array_equal(got[m], new[k][m]), (p, k, m)
        assert np.array_equal(out["mse_center"], ref_mse_center)
        # the field without stamps is unchanged and has no field_mse
        for k in ("work", "final", "mean", "stddev"):
            assert np.array_equal(new[k][1], state[k][1])
        assert np.isnan(out["field_mse"][1])
        n = F * F * NB
        for m in (0, 2, 3, 4):
            assert _mse_close(out["field_mse"][m], mse(state["work"][m], new["work"][m]), n), (p, m)
        if cumulative:
            assert np.array_equal(new["work"], new["final"])
        elif p == 1:
            assert not np.array_equal(new["work"][0], new["final"][0])
        state = new
    assert np.abs(state["mean"][0]).max() > 0
    fs.close()


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_field_mse_is_reproducible_and_independent_of_the_other_fields(dtype):
    from debvader_amd.training.metrics import mse

    net = _net(dtype)
    eng = net._core.engine
    F = 131
    fields = _blob_fields(3, F, seed=21)
    starts, places, fp = _case(F, [20, 9, 33], seed=8, hang=False)

    def run(flds, st, pl, fptr):
        fs = eng.open_field_set(flds, cumulative=True)
        before = fs.read("work")
        out = fs.deblend_pass(st, pl, fptr, seed=5)
        after = fs.read("work")
        fs.close()
        return out["field_mse"], before, after

    a, before, after = run(fields, starts, places, fp)
    n = F * F * NB
    for m in range(3):
        assert _mse_close(a[m], mse(before[m], after[m]), n), m
    b, _, _ = run(fields, starts, places, fp)
    assert a.tobytes() == b.tobytes()                              # a rerun: the same bits
    # the field stays first (its noise rows do not move); the others are replaced, and there are more of them
    others = _blob_fields(4, F, seed=99)
    others[0] = fields[0]
    st2, pl2, fp2 = _case(F, [20, LOTS, 0, 5], seed=31, hang=False)
    st2[:20], pl2[:20] = starts[:20], places[:20]
    c, _, after2 = run(others, st2, pl2, fp2)
    assert np.array_equal(after2[0], after[0])
    assert a[:1].tobytes() == c[:1].tobytes() and a[1] != c[1]
    assert np.isnan(c[2])


LOTS = 70          # more stamps than one chunk of max_batch = 64


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_detection_on_the_resident_residual(dtype):
    net = _net(dtype)
    ctx, eng = net._core.ctx, net._core.engine
    F = 131
    fields = _blob_fields(5, F, seed=11)
    starts, places, fp = _case(F, COUNTS, seed=5, hang=False)
    fs = eng.open_field_set(fields, cumulative=False)
    fs.deblend_pass(starts, places, fp, seed=3)
    work = fs.read("work")
    assert not np.array_equal(work[0], fields[0])
    for active in (None, np.array([True, False, True, True, False])):
        got = fs.detect(active=active)
        on = np.ones(5, bool) if active is None else active
        ref = ctx.scene_detect(work[on][:, :, :, 2])
        idx = np.nonzero(on)[0]
        exp_off = np.zeros(6, np.int64)
        for a, m in enumerate(idx):
            exp_off[m + 1] = ref["offsets"][a + 1] - ref["offsets"][a]
        exp_off = np.cumsum(exp_off)
        assert np.array_equal(got["offsets"], exp_off)
        assert len(got["x"]) == len(ref["x"]) > 0
        for k in ("x", "y", "npix", "parent", "peak", "flux"):
            assert got[k].tobytes() == ref[k].tobytes(), k
        assert np.array_equal(got["field"], idx[ref["field"]])
        assert np.array_equal(got["globalrms"][on], ref["globalrms"]) and not got["globalrms"][~on].any()
    fs.close()


def test_detection_one_field_per_launch_gives_the_same_bytes():
    """three resident 72-pixel fields (a set's fields are square; 4.5 meshes of 16 px a side), a few sources each, the middle
    one inactive in half of the calls: detect() with the default workspace (one launch) against a workspace that holds exactly
    one field (one launch per active field, the set's field numbers read at an offset), every output, in each mode the set can
    hold: band 2 alone, single-band planes, a band selection without and with planes, and the object columns with the segmap"""
    import re

    from debvader_amd._lib import DvError

    net = _net("float32")
    eng = net._core.engine
    F = 72
    rng = np.random.default_rng(23)
    y, x = np.mgrid[:F, :F]
    fields = rng.normal(0, 0.05, (3, F, F, NB))
    for i, srcs in enumerate((((12, 10), (30, 50), (60, 8)), ((8, 30), (44, 20)), ((20, 12), (36, 60), (10, 34)))):
        for cy, cx in srcs:
            g = np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / 1.8 ** 2)
            fields[i] += g[:, :, None] * rng.uniform(2.0, 6.0, NB)
    w = rng.uniform(200.0, 600.0, (3, F, F, NB))
    w[:, :, 40, :] = 0.0
    fs = eng.open_field_set(fields)

    def both():
        for active in (None, np.array([True, False, True])):
            kw = dict(active=active, thresh=3.0, back_size=16)
            a = fs.detect(**kw)
            on = np.ones(3, bool) if active is None else active
            assert (np.diff(a["offsets"])[on] >= 2).all() and not np.diff(a["offsets"])[~on].any()
            with pytest.raises(DvError, match="workspace") as refused:
                fs.detect(workspace_bytes=1, **kw)
            need = int(re.search(r"needs up to (\d+) bytes", str(refused.value)).group(1))
            b = fs.detect(workspace_bytes=need, **kw)
            assert set(a) == set(b)
            for k in a:
                assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        return a

    assert "segmap" not in both()                           # band 2 alone
    fs.set_detect_weights(w[..., 2])
    both()
    fs.set_detect_weights(None)
    fs.set_detect_bands((4, 1, 2), band_weights=(1.0, 0.5, 2.0))
    both()
    fs.set_detect_bands((5, 0), weights=w[..., [5, 0]], noise="absolute", filter_type="matched")
    both()
    fs.set_detect_objects(True, segmentation_map=True)
    last = both()
    assert last["segmap"].shape == (3, F, F) and last["segmap"][0].any() and not last["segmap"][1].any()
    fs.close()


def _loop_fields():
    """Six 131-pixel fields for the loop tests: blob fields of different crowding and brightness, and one of pure noise."""
    F = 131
    f = np.concatenate([_blob_fields(1, F, seed=41, nblob=3), _blob_fields(1, F, seed=42, nblob=8),
                        _blob_fields(1, F, seed=43, nblob=14, amp=(0.5, 4.0)), _blob_fields(1, F, seed=44, nblob=20),
                        _blob_fields(1, F, seed=45, nblob=6, amp=(6.0, 30.0))])
    noise = np.random.default_rng(46).normal(0, 0.05, size=(1, F, F, NB))
    return np.concatenate([f[:2], noise, f[2:]])


NOISE_FIELD = 2


def _loop_net(dtype):
    """The net of the loop tests.  Freshly initialised weights predict stamps that are nearly zero, so a residual would be
    the field again and every field would make the same passes; a bias of 1 on the head's six mean channels makes every
    stamp remove about one unit of flux per pixel, faint galaxies drop below the detection threshold before bright ones,
    and the fields stop after different numbers of passes (on an MI355X, both engines: 2, 2, 0, 1, 2, 2 passes in reference
    mode and 4, 6, 0, 1, 2, 8 in cumulative mode)."""
    net = _net(dtype)
    eng = net._core.engine
    bias = eng.get_param("dec/head/bias")
    bias[:NB] = 1.0
    eng.set_param("dec/head/bias", bias)
    return net


def _restated_loop(net, fields, mode, mse_criterion=100.0, max_iterations=None):
    """The rules of IterativeDeblendFieldBatch driven from the host with the calls that exist without the set."""
    from debvader_amd.deblend.field_deblender import batch_windows
    from debvader_amd.detect.detection import detect_objects_batch
    from debvader_amd.training.metrics import mse

    core = net._core
    ctx, eng = core.ctx, core.engine
    M, F = fields.shape[:2]
    cumulative = mode == "cumulative"
    if cumulative and max_iterations is None:
        max_iterations = 10
    st = _initial(fields)
    active, prev, total = [True] * M, [0] * M, [0] * M
    rows, mses = [[] for _ in range(M)], [[] for _ in range(M)]
    k = 0
    while any(active) and (max_iterations is None or k < max_iterations):
        idx = [m for m in range(M) if active[m]]
        dist = [np.zeros((0, 2))] * M
        for m, d in zip(idx, detect_objects_batch(st["work"][idx], ctx=ctx)):
            dist[m] = d
        starts, fp, kept, dd = batch_windows(F, dist, CS)
        if len(starts) == 0:
            break
        places = (int((F - CS) / 2) + dd).astype(np.int64)
        seed = core.next_seed()
        mse_center = eng.infer_fields_composite(st["work"], starts, places, fp, seed=seed)["mse_center"]
        new = _expected_pass(net, st, starts, places, fp, seed, cumulative)
        for m in idx:
            lo, hi = int(fp[m]), int(fp[m + 1])
            if hi == lo:
                active[m] = False
                continue
            for i in range(hi - lo):
                rows[m].append((int(kept[m][i]) + total[m], dd[lo + i, 0], dd[lo + i, 1], mse_center[lo + i],
                                not mse_center[lo + i] > mse_criterion, k))
            mses[m].append(mse(st["work"][m], new["work"][m]))
            total[m] += hi - lo
            if not cumulative and not hi - lo > prev[m]:
                active[m] = False
            prev[m] = hi - lo
        st = new
        k += 1
    return rows, mses, st


def _rows_of(rec):
    return [(int(r["list_idx"]), float(r["galaxy_distances_to_center_x"]), float(r["galaxy_distances_to_center_y"]),
             float(r["mse_center"]), bool(r["passed_cuts"]), int(r["iteration"])) for r in rec]


@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_the_class_against_a_host_driven_restatement(dtype, mode):
    from debvader_amd.deblend_iterative import IterativeDeblendFieldBatch

    net = _loop_net(dtype)
    fields = _loop_fields()
    M, F = fields.shape[:2]
    n = F * F * NB
    net._core.seed_counter = 500
    exp_rows, exp_mse, exp = _restated_loop(net, fields, mode)
    seeds_used = net._core.seed_counter - 500
    net._core.seed_counter = 500
    it = IterativeDeblendFieldBatch(net, fields)
    res = it.iterative_deblending(mode=mode)
    assert net._core.seed_counter - 500 == seeds_used
    passes = [len(m) for m in it.mse]
    print(f"{dtype} {mode}: passes per field {passes}, galaxies per field {[len(r) for r in res]}")
    for m in range(M):
        got = _rows_of(res[m])
        assert len(got) == len(exp_rows[m]), m
        for g, e in zip(got, exp_rows[m]):
            assert g[:3] == e[:3] and g[4:] == e[4:], (m, g, e)
            assert np.float64(g[3]).tobytes() == np.float64(e[3]).tobytes(), (m, g, e)     # (NaN-proof equality)
        assert all(np.array_equal(s, [0, 0]) for s in res[m]["shifts"])
        assert len(it.mse[m]) == len(exp_mse[m]), m
        for a, b in zip(it.mse[m], exp_mse[m]):
            assert _mse_close(a, b, n), (m, a, b)
    assert np.array_equal(it.get_residual_fields(), exp["final"])
    pred = it.get_predicted_fields()
    assert np.array_equal(pred["predicted_mean_fields"], exp["mean"])
    assert np.array_equal(pred["predicted_stddev_fields"], exp["stddev"])
    # the inputs are not vacuous
    assert max(passes) >= 2
    assert passes[NOISE_FIELD] == 0 and len(res[NOISE_FIELD]) == 0
    if mode == "cumulative":
        assert len({p for p in passes if p > 0}) >= 2          # fields that iterate stop after different numbers of passes
    assert [sum(1 for c in col if c > 0) for col in zip(*it.nb_of_deblended_galaxies)] == passes


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_one_field_against_the_single_field_class(dtype):
    from debvader_amd.deblend_iterative import IterativeDeblendField, IterativeDeblendFieldBatch

    net = _loop_net(dtype)
    fields = _loop_fields()
    F = fields.shape[1]
    n = F * F * NB
    compared_residual = 0
    for m in (0, 1, 3):
        net._core.seed_counter = 900
        single = IterativeDeblendField(net, fields[m:m + 1])
        rec = single.iterative_deblending()
        net._core.seed_counter = 900
        batch = IterativeDeblendFieldBatch(net, fields[m:m + 1])
        res = batch.iterative_deblending(mode="reference")[0]
        assert len(res) > 0 and len(rec) >= len(res)
        for k in ("list_idx", "galaxy_distances_to_center_x", "galaxy_distances_to_center_y", "passed_cuts"):
            assert np.array_equal(np.asarray(rec[k][:len(res)]), res[k]), (m, k)
        assert len(single.mse) >= len(batch.mse[0]) >= 1
        for a, b in zip(batch.mse[0], single.mse):
            assert _mse_close(a, b, n), (m, a, b)
        ended_on_empty_pass = len(single.mse) > len(single.nb_of_deblended_galaxies)
        print(f"{dtype} field {m}: {len(batch.mse[0])} passes, single-field class ended on an empty pass: {ended_on_empty_pass}")
        if not ended_on_empty_pass:
            assert len(rec) == len(res) and len(single.mse) == len(batch.mse[0])
            # after iterative_deblending() the single-field class holds the concatenated records of ALL its passes in
            # res_deblend, and get_residual_field() subtracts their stamps from the field in that order: the field minus
            # every galaxy of every pass, which is the set's `final` - for any number of passes, not only for one
            assert np.array_equal(single.get_residual_field()[0], batch.get_residual_fields()[0]), m
            compared_residual += 1
    assert compared_residual >= 1


def test_refusals_leave_the_set_and_the_engine_usable(monkeypatch):
    from debvader_amd._lib import DvError, lib

    net = _net("float32")
    eng = net._core.engine
    F = 131
    fields = _blob_fields(3, F, seed=11)
    starts, places, fp = _case(F, [10, 0, 20], seed=5, hang=False)
    state = _initial(fields)
    expected = _expected_pass(net, state, starts, places, fp, 9, False)
    plain = eng.infer_fields(fields, starts, fp, seed=9)

    fs = eng.open_field_set(fields)
    bad = starts.copy()
    bad[3] = (F - CS + 1, 0)
    with pytest.raises(DvError, match="leaves the 131-pixel field") as e:
        fs.deblend_pass(bad, places, fp, seed=9)
    assert e.value.status == -1
    with pytest.raises(ValueError, match="field_ptr"):
        fs.deblend_pass(starts, places, [0, 10, 30], seed=9)
    fp_bad = np.array([0, 10, 10, 29], np.int64)               # past the binding's own check, to the library's
    mc, fm = np.zeros(30), np.zeros(3)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    s32, p32 = starts.astype(np.int32), places.astype(np.int32)
    assert lib.dv_field_set_pass(fs._h, s32.ctypes.data_as(ip), p32.ctypes.data_as(ip),
                                 fp_bad.ctypes.data_as(C.POINTER(C.c_int64)), 30, 9, mc.ctypes.data_as(dp),
                                 fm.ctypes.data_as(dp)) == -1
    # a budget below the set's six buffers per field: refused with the bytes needed and available in the message
    monkeypatch.setenv("DV_FIELDS_GROUP_MB", "4")
    with pytest.raises(DvError, match=r"need \d+ bytes.*4194304 bytes are available") as e:
        eng.open_field_set(fields)
    assert e.value.status == -3
    monkeypatch.delenv("DV_FIELDS_GROUP_MB")
    # the refused calls changed nothing: the set still holds the fields, and a pass gives the expected bits
    assert np.array_equal(fs.read("work"), fields) and not fs.read("mean").any()
    fs.deblend_pass(starts, places, fp, seed=9)
    for k in ("work", "final", "mean", "stddev"):
        assert np.array_equal(fs.read(k), expected[k]), k
    # a closed set: the binding and the library both refuse
    raw = C.c_void_p(fs._h.value)
    fs.close()
    with pytest.raises(DvError, match="closed"):
        fs.read("work")
    out = np.zeros(fields.shape)
    assert lib.dv_field_set_read(raw, 0, out.ctypes.data_as(dp)) == -5
    assert lib.dv_field_set_close(raw) == -5
    assert lib.dv_field_set_pass(raw, s32.ctypes.data_as(ip), p32.ctypes.data_as(ip), fp.ctypes.data_as(C.POINTER(C.c_int64)),
                                 30, 9, mc.ctypes.data_as(dp), fm.ctypes.data_as(dp)) == -5
    # afterwards: a pass on a fresh set and an ordinary infer_fields call give the expected bits
    fs2 = eng.open_field_set(fields)
    fs2.deblend_pass(starts, places, fp, seed=9)
    for k in ("work", "final", "mean", "stddev"):
        assert np.array_equal(fs2.read(k), expected[k]), k
    fs2.close()
    again = eng.infer_fields(fields, starts, fp, seed=9)
    assert np.array_equal(again["loc"], plain["loc"]) and np.array_equal(again["scale"], plain["scale"])
