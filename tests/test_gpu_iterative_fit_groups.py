"""The joint flux fit of all passes by blend groups, in place on the stamp store of a resident field set
(dv_field_set_fit_flux_groups, FieldSet.fit_flux_groups, IterativeDeblendFieldBatch.iterative_catalogue(fit_flux=True,
fit_groups=True)).  Expected values never come from the code under test: Context.scene_fit_flux_groups
gets the mean stamps Engine.infer_fields returns for every pass's working residual, regrouped field by field by the index
arithmetic of tests/test_gpu_iterative_fit_flux.py, and the uploaded fields as the data; the groups come from the union-find
of tests/fit_flux_groups_oracle.py on the joint placements.  Every comparison of the fit is bit for bit: the kernels are the
ones of the stand-alone call, and reading a stamp through the row table gives the values a copy of it gives.  The network is
the 31-pixel one of tests/test_gpu_blend.py, both engines."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import fit_flux_groups_oracle as fgo
from tests.test_gpu_blend import COUNTS, CS, F2, NB, _blob_fields, _eq, _net, _windows
from tests.test_gpu_iterative_catalogue import STACKS, _loop_net
from tests.test_gpu_iterative_fit_flux import _case, _measured_set, _stamps

pytestmark = pytest.mark.gpu

KEYS = ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status")
WKEYS = KEYS + ("fit_chi2", "fit_npix")
GKEYS = ("fit_group", "fit_group_size")


def _order(fps):
    """order[dst] = resident row, field by field, pass after pass inside a field; and the joint field_ptr"""
    M = len(fps[0]) - 1
    n0 = np.concatenate([[0], np.cumsum([int(fp[-1]) for fp in fps])])
    order = np.concatenate([np.arange(n0[p] + fp[m], n0[p] + fp[m + 1]) for m in range(M) for p, fp in enumerate(fps)])
    counts = np.sum([np.diff(fp) for fp in fps], axis=0)
    return order.astype(np.int64), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _same(got, want, order, what, keys=None):
    """got: the set's call, rows in call order; want: the stand-alone call on the regrouped rows"""
    assert sorted(got) == sorted(want), what
    for k in (keys or want):
        assert got[k].dtype == want[k].dtype and _eq(got[k][order], want[k]), (what, k)


# ---- 1: the bits of the stand-alone call, of the dense joint fit, and the groups of the restatement ------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_the_grouped_joint_fit_has_the_bits_of_the_standalone_call_and_of_the_dense_joint_fit(dtype, mode, weighted):
    c = _case(dtype, mode)
    assert np.diff(c["fp_all"]).tolist() == [60, 0, 300, 14, 80]
    W = c["W"] if weighted else None
    data = c["data"] if weighted else c["fields"]                   # (the NaN pixel needs its zero weight)
    want = c["ctx"].scene_fit_flux_groups(c["stamps"], c["places"], data, field_ptr=c["fp_all"], weight_fields=W)
    got = c["fs"].fit_flux_groups(data_fields=data, weight_fields=W)
    assert sorted(got) == sorted((WKEYS if weighted else KEYS) + GKEYS)
    _same(got, want, c["order"], "stand-alone")
    assert got["fit_scale"].shape == (2 * sum(COUNTS), NB) and got["fit_group"].shape == (2 * sum(COUNTS),)
    # section 7w's bit-identity carries over: every shared column is the dense joint fit's, in call order
    dense = c["fs"].fit_flux(data_fields=data, weight_fields=W)
    for k in dense:
        assert got[k].dtype == dense[k].dtype and _eq(got[k], dense[k]), ("dense", k)
    # the groups: the restatement on the joint placements
    group, size = fgo.groups(c["places"], c["fp_all"], CS, F2)
    assert _eq(got["fit_group"][c["order"]], group) and _eq(got["fit_group_size"][c["order"]], size)
    st = got["fit_status"]
    print(f"[{dtype} {mode} {'weighted' if weighted else 'plain'}] status 0 / 4 / 5: {int((st == 0).sum())} / {int((st == 4).sum())} / "
          f"{int((st == 5).sum())} of {st.size} (row, band) pairs; groups per field "
          f"{[len(np.unique(group[a:b])) for a, b in zip(c['fp_all'][:-1], c['fp_all'][1:])]}, largest {int(size.max())}")
    assert (st == 0).sum() >= st.size // 2                         # the system is not vacuous
    if not weighted and not c["cumulative"]:                       # the resident base is the uploaded fields
        base = c["fs"].fit_flux_groups()
        assert all(base[k].tobytes() == got[k].tobytes() for k in got)


# ---- 2: a field of 1200 rows over two passes ----------------------------------------------------------------------------------
F3, PITCH, BOX, PER_PASS = 259, 64, 20, 600
KEPT_PIVOT = 0.5     # the pivot bound of the comparison with numpy (its docstring says why)


def _cluster_windows(seed):
    """600 windows of one 259-pixel field in 16 clusters: window i belongs to cluster i % 16, whose starts lie in a box of 20
    pixels at (64 a, 64 b); the stamps go back where they were cut"""
    rng = np.random.default_rng(seed)
    k = np.arange(PER_PASS) % 16
    starts = (np.stack([PITCH * (k // 4), PITCH * (k % 4)], axis=1) + rng.integers(0, BOX, size=(PER_PASS, 2))).astype(np.int32)
    return starts, starts.copy(), np.array([0, PER_PASS], np.int64)


def _field_259(seed):
    rng = np.random.default_rng(seed)
    out = rng.normal(0, 0.05, size=(1, F3, F3, NB))
    yy, xx = np.mgrid[:F3, :F3]
    for _ in range(60):
        r, c = rng.uniform(10, F3 - 10, size=2)
        sig, a = rng.uniform(1.5, 3.0), rng.uniform(2.0, 9.0)
        out[0] += (a * np.exp(-0.5 * ((yy - r) ** 2 + (xx - c) ** 2) / sig ** 2))[:, :, None] * rng.uniform(0.5, 1.0, size=NB)
    return out


@functools.lru_cache(maxsize=None)
def _cluster_case(dtype):
    """Two measured passes of 600 windows each on the 16-cluster field, the grouped joint fit of the set at the default pivot
    bound and at KEPT_PIVOT, the stand-alone calls on the re-derived stamps, and what the dense joint fit says to 1200 rows; the set is closed, nothing here is written to"""
    from debvader_amd._lib import DvError

    net = _net(dtype)
    eng, ctx = net._core.engine, net._core.ctx
    field = _field_259(23)
    windows, seeds = [_cluster_windows(61), _cluster_windows(62)], [81, 82]
    places = np.concatenate([w[1] for w in windows])
    fs, _, _, works = _measured_set(eng, field, False, windows, seeds)
    try:
        stamps = _stamps(eng, works, windows, seeds)
        sums = fs.blend_sums()
        try:
            fs.fit_flux()
            refusal = None
        except DvError as e:
            refusal = str(e)
        usable = _eq(fs.blend_sums(), sums)                         # the set still answers, with the same bits
        got = fs.fit_flux_groups()
        got_kept = fs.fit_flux_groups(min_pivot=KEPT_PIVOT)
    finally:
        fs.close()
    order, fp_all = _order([w[2] for w in windows])
    want = ctx.scene_fit_flux_groups(stamps, places, field, field_ptr=fp_all)
    want_kept = ctx.scene_fit_flux_groups(stamps, places, field, field_ptr=fp_all, min_pivot=KEPT_PIVOT)
    return dict(ctx=ctx, field=field, stamps=stamps, places=places, order=order, fp_all=fp_all, got=got, want=want,
                got_kept=got_kept, want_kept=want_kept, refusal=refusal, usable=usable)


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_a_field_of_1200_rows_in_16_clusters(dtype):
    c = _cluster_case(dtype)
    places, got = c["places"], c["got"]
    # the clusters cannot touch: every stamp ends before the next box begins, in both directions
    cell = places // PITCH
    assert (places >= 0).all() and (places + CS <= F3).all() and (places - PITCH * cell + CS <= PITCH).all()
    assert (cell[:, 0] * 4 + cell[:, 1] == np.tile(np.arange(PER_PASS) % 16, 2)).all() and BOX + CS <= PITCH
    assert c["order"].tolist() == list(range(2 * PER_PASS)) and c["fp_all"].tolist() == [0, 2 * PER_PASS]
    # the dense joint fit refuses the field, and the set stays usable
    assert c["refusal"] is not None and "field 0 has 1200 galaxies" in c["refusal"] and c["usable"]
    _same(got, c["want"], c["order"], "1200 rows")
    group, size = fgo.groups(places, c["fp_all"], CS, F3)
    assert _eq(got["fit_group"], group) and _eq(got["fit_group_size"], size)
    # (600 = 16 x 37.5: clusters 0 - 7 hold 38 stamps per pass, the others 37; inside a box every pair of stamps overlaps)
    assert np.unique(group).tolist() == list(range(16))
    assert size.tolist() == [76 if (k % PER_PASS) % 16 < 8 else 74 for k in range(2 * PER_PASS)]
    assert (got["fit_status"] == 0).sum() >= got["fit_status"].size // 2


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_the_groups_of_that_field_against_numpy_on_the_gpus_own_gram_blocks(dtype):
    """Section 7q's bounds against numpy on the Gram blocks dv_scene_fit_flux_gram returns for every group, under their
    condition: a scaled condition number of every group's KEPT system below 100, asserted first.

    The fit is the one at KEPT_PIVOT = 0.5: a row stays in its system only while at least half of its model's norm is not
    explained by the rows before it - the earlier pass first.  At the default bound of 1e-8 nothing is dropped here, "kept"
    says nothing, and the condition cannot hold: the stamps of a freshly initialised network hardly depend on the pixels they
    are cut from (a field of zeros gives the same figures), so a group is 75 overlapping copies of one pattern per band inside
    a 20-pixel box, with scaled condition numbers of 9.3 to 4128 over the 96 systems (median 135; the bounds hold there too,
    worst fractions 1.5e-06, 4.2e-04, 3.7e-05, but not under their condition).  The pivot bound is the fit's own means of
    keeping a system it can solve, and which rows it keeps has the bits of the stand-alone call, checked below.  Measured at
    0.5: the largest condition number per band is 59 / 61 / 13 / 19 / 17 / 60 on both engines, 3 to 76 rows are kept per
    system and 3050 of the 7200 (row, band) pairs are dropped, so h' = h - sum of the dropped columns is part of every
    comparison; the worst fractions of the bounds were backward 2.4e-06, scale 4.3e-05, var 2.3e-06."""
    c = _cluster_case(dtype)
    ctx, got, stamps, places, field = c["ctx"], c["got_kept"], c["stamps"], c["places"], c["field"]
    _same(got, c["want_kept"], c["order"], "1200 rows at the pivot bound of the kept systems")
    group = got["fit_group"]
    assert _eq(group, c["got"]["fit_group"]) and (got["fit_status"] == 5).any()      # (the groups are geometry alone)
    worst = dict(backward=0.0, scale=0.0, var=0.0)
    conds = np.zeros((16, NB))
    for gi, root in enumerate(np.unique(group)):
        rows = np.nonzero(group == root)[0]
        g = ctx.scene_fit_flux_gram(stamps[rows], places[rows], field[0])
        for b in range(NB):
            A = np.tril(g["gram"][b]) + np.tril(g["gram"][b], -1).T
            assert np.array_equal(np.diagonal(A), got["fit_gram"][rows, b]) and np.array_equal(g["proj"][:, b], got["fit_proj"][rows, b])
            st = got["fit_status"][rows, b]
            kept, dropped = st == 0, st == 5
            assert kept.sum() >= 2 and not (st == 4).any()
            A, h = A[np.ix_(kept, kept)], g["proj"][kept, b] - A[np.ix_(kept, dropped)].sum(axis=1)
            d = 1.0 / np.sqrt(np.diagonal(A))
            conds[gi, b] = np.linalg.cond(A * d[:, None] * d[None, :])
            a, v = got["fit_scale"][rows[kept], b], got["fit_var"][rows[kept], b]
            sol, wv = np.linalg.solve(A, h), np.diagonal(np.linalg.inv(A))
            back, bound = np.abs(A @ a - h).max(), 1e-10 * (np.abs(A).sum(axis=1).max() * np.abs(a).max() + np.abs(h).max())
            worst["backward"] = max(worst["backward"], back / bound)
            worst["scale"] = max(worst["scale"], np.abs(a - sol).max() / (1e-10 * np.abs(sol).max()))
            worst["var"] = max(worst["var"], (np.abs(v - wv) / wv).max() / 1e-9)
    print(f"[{dtype}] 16 groups of 74 or 76 rows, {NB} bands: scaled condition numbers of the kept systems {conds.min():.1f} .. "
          f"{conds.max():.1f}, median {np.median(conds):.1f}, largest per band {np.round(conds.max(axis=0), 1).tolist()}, "
          f"{int((conds < 100.0).sum())} of {conds.size} below 100; rows dropped {int((got['fit_status'] == 5).sum())}")
    print(f"[{dtype}] worst fraction of each bound - " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert conds.max() < 100.0                                      # the condition of the bounds: a condition, not a measurement
    assert worst["backward"] <= 1.0 and worst["scale"] <= 1.0 and worst["var"] <= 1.0


# ---- 3: a stamp of pass 1 that joins two groups of pass 0 ---------------------------------------------------------------------
def test_a_stamp_of_the_second_pass_joins_two_groups_of_the_first():
    """Field 1, pass 0: C at (90, 90) alone, A at (10, 10) and B at (10, 70), 29 columns apart.  Pass 1: X at (20, 40) shares
    column 40 with A and column 70 with B; Y at (90, 10) is alone.  Field 0 holds two stamps in pass 0 and one in pass 1, so the
    joint order is not the resident order."""
    net = _net("float32")
    eng, ctx = net._core.engine, net._core.ctx
    fields = _blob_fields(2, seed=11)
    i32 = lambda a: np.array(a, np.int32)
    windows = [(i32([(5, 5), (60, 60), (90, 90), (10, 10), (10, 70)]), i32([(5, 5), (60, 60), (90, 90), (10, 10), (10, 70)]),
                np.array([0, 2, 5], np.int64)),
               (i32([(40, 40), (20, 40), (90, 10)]), i32([(40, 40), (20, 40), (90, 10)]), np.array([0, 1, 3], np.int64))]
    seeds = [71, 72]
    fs, _, _, works = _measured_set(eng, fields, False, windows, seeds)
    try:
        stamps = _stamps(eng, works, windows, seeds)
        places = np.concatenate([w[1] for w in windows])
        order, fp_all = _order([w[2] for w in windows])
        assert order.tolist() == [0, 1, 5, 2, 3, 4, 6, 7] and fp_all.tolist() == [0, 3, 8]
        got = fs.fit_flux_groups()
        # in call (resident) order: pass 0 = field 0 (2 rows), field 1 (C, A, B); pass 1 = field 0 (1 row), field 1 (X, Y)
        assert got["fit_group"][[2, 3, 4, 6, 7]].tolist() == [0, 1, 1, 1, 4]
        assert got["fit_group_size"][[2, 3, 4, 6, 7]].tolist() == [1, 3, 3, 3, 1]
        group, size = fgo.groups(places[order], fp_all, CS, F2)
        assert _eq(got["fit_group"][order], group) and _eq(got["fit_group_size"][order], size)
        _same(got, ctx.scene_fit_flux_groups(stamps[order], places[order], fields, field_ptr=fp_all), order, "bridge")
        # pass 0 alone has A and B in groups of their own
        alone = ctx.scene_fit_groups(places[:5], CS, F2, field_ptr=windows[0][2])
        assert alone["fit_group"][2:].tolist() == [0, 1, 2] and alone["fit_group_size"][2:].tolist() == [1, 1, 1]
    finally:
        fs.close()


# ---- 4: rows dropped, reruns, independence, the scratch ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_a_pivot_bound_that_drops_rows_of_the_later_pass(dtype):
    c = _case(dtype, "reference")
    loose = c["fs"].fit_flux_groups(min_pivot=0.3)
    _same(loose, c["ctx"].scene_fit_flux_groups(c["stamps"], c["places"], c["fields"], field_ptr=c["fp_all"], min_pivot=0.3),
          c["order"], "min_pivot 0.3")
    n0 = sum(COUNTS)
    st = loose["fit_status"]
    # the twins: field 3's second pass repeats the windows of its first, row for row
    lo, hi = int(c["windows"][0][2][3]), int(c["windows"][0][2][4])
    assert np.array_equal(c["windows"][0][1][lo:hi], c["windows"][1][1][lo:hi]) and hi - lo == 7
    early, late = st[lo:hi], st[n0 + lo:n0 + hi]
    print(f"[{dtype}] min_pivot 0.3: {int((st == 5).sum())} (row, band) pairs dropped, {int((st[:n0] == 5).sum())} of them in pass 0; "
          f"of the twins of field 3 {int((early == 5).sum())} in pass 0 and {int((late == 5).sum())} in pass 1")
    assert (st == 5).any()
    assert not (early == 5).any()                                   # a dropped row whose twin is in the set is the later one
    assert (loose["fit_scale"][st == 5] == 1.0).all()


@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_rerun_independence_and_the_scratch(dtype):
    from debvader_amd._lib import DvError

    c = _case(dtype, "reference")
    fs, eng = c["fs"], c["eng"]
    first = fs.fit_flux_groups(data_fields=c["data"], weight_fields=c["W"])
    again = fs.fit_flux_groups(data_fields=c["data"], weight_fields=c["W"])
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)
    # a scratch that holds the largest group and no more: every group above half of it goes through it alone
    plain = fs.fit_flux_groups()
    largest = int(plain["fit_group_size"].max())
    need = NB * largest * largest * 8
    assert largest >= 100
    tight = fs.fit_flux_groups(scratch_bytes=need)
    assert all(plain[k].tobytes() == tight[k].tobytes() for k in plain)
    row = int(np.nonzero(plain["fit_group_size"][c["order"]] == largest)[0][0])
    f = int(np.searchsorted(c["fp_all"], row, side="right") - 1)
    with pytest.raises(DvError, match=rf"dv_field_set_fit_flux_groups: field {f}: the blend group of row {row - int(c['fp_all'][f])} has "
                                      rf"{largest} galaxies: its Gram matrices need {need} bytes of scratch .* scratch_bytes is {need - 1}"):
        fs.fit_flux_groups(scratch_bytes=need - 1)
    after = fs.fit_flux_groups()
    assert all(plain[k].tobytes() == after[k].tobytes() for k in plain)
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
    moved = fs2.fit_flux_groups()
    fs2.close()
    n0, n1 = sum(COUNTS), sum(counts)
    for k in KEYS + GKEYS:
        for p in range(2):
            assert moved[k][p * n1:p * n1 + 30].tobytes() == plain[k][p * n0:p * n0 + 30].tobytes(), (k, p)


def test_the_stamp_store_grows_with_the_rows():
    """227 + 227 + 600 rows cross the first capacity of 1024: the stamps of the first two passes are copied over, and the row
    table still finds every one of them"""
    c = _case("float32", "reference")
    eng, ctx = c["eng"], c["ctx"]
    windows = c["windows"] + [_windows([250, 0, 150, 100, 100], seed=19)]
    seeds = c["seeds"] + [79]
    fs, _, _, works = _measured_set(eng, c["fields"], False, windows, seeds)
    try:
        stamps = _stamps(eng, works, windows, seeds)
        order, fp_all = _order([w[2] for w in windows])
        assert len(order) == 1054 and np.diff(fp_all).tolist() == [310, 0, 450, 114, 180]
        places = np.concatenate([w[1] for w in windows])
        want = ctx.scene_fit_flux_groups(stamps[order], places[order], c["fields"], field_ptr=fp_all)
        _same(fs.fit_flux_groups(), want, order, "three passes")
    finally:
        fs.close()


# ---- 5: the refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_set_usable():
    from debvader_amd import _lib
    from debvader_amd.engine import _dp, _ip

    DvError, lib = _lib.DvError, _lib.lib
    c = _case("float32", "reference")
    fs, eng, fields = c["fs"], c["eng"], c["fields"]
    n = 2 * sum(COUNTS)
    want = fs.fit_flux_groups()
    before = {k: fs.read(k) for k in STACKS}
    sums = fs.blend_sums()
    o = [np.zeros((n, NB)) for _ in range(4)] + [np.zeros((n, NB), np.int32)]
    grp = [np.zeros(n, np.int32), np.zeros(n, np.int32)]
    par = _lib.DvFitFluxParams(1e-8, 256 << 20)

    def raw(h=None, rows=n, par_=par, chi=(None, None), groups=None):
        ptrs = [_dp(a) for a in o[:4]] + [_ip(o[4])]
        g = [_ip(a) for a in grp] if groups is None else groups
        return lib.dv_field_set_fit_flux_groups(h or fs._h, rows, None, None, C.byref(par_) if par_ else None, *ptrs, *chi, *g)

    assert raw() == 0 and all(_eq(a, want[k]) for a, k in zip(o + grp, KEYS + GKEYS))
    assert raw(rows=n + 1) == -1 and "resident rows" in _lib.last_error()
    assert raw(par_=None) == -1 and "params" in _lib.last_error()
    assert raw(par_=_lib.DvFitFluxParams(1.5, 256 << 20)) == -1 and "min_pivot" in _lib.last_error()
    assert raw(par_=_lib.DvFitFluxParams(1e-8, 0)) == -1 and "scratch_bytes" in _lib.last_error()
    assert raw(chi=(_dp(o[0]), _ip(o[4]))) == -1 and "fit_chi2" in _lib.last_error()      # chi-square outputs without weights
    assert raw(groups=[None, None]) == -1 and "fit_group" in _lib.last_error()
    for bad in (dict(min_pivot=0.0), dict(scratch_bytes=0), dict(data_fields=fields[:, :-1]), dict(weight_fields=fields[:2])):
        with pytest.raises(ValueError):
            fs.fit_flux_groups(**bad)
    # a set that never kept its stamps, and NULL data on a cumulative set
    bare = eng.open_field_set(fields)
    bare.deblend_pass_measure(*c["windows"][0], seed=77)
    with pytest.raises(DvError, match="keeps no stamps"):
        bare.fit_flux_groups()
    assert bare.blend_sums().shape == (n // 2, 4)                               # (the set still answers)
    bare.close()
    cum = _case("float32", "cumulative")
    with pytest.raises(ValueError, match="cumulative"):
        cum["fs"].fit_flux_groups()
    assert raw(h=cum["fs"]._h) == -1 and "cumulative" in _lib.last_error()
    # nothing moved: the stacks, the rows and the fit are what they were
    for k in STACKS:
        assert np.array_equal(fs.read(k), before[k]), k
    assert _eq(fs.blend_sums(), sums)
    after = fs.fit_flux_groups()
    assert all(after[k].tobytes() == want[k].tobytes() for k in want)
    # a closed set: the binding and the library both refuse
    gone = eng.open_field_set(fields[:1])
    handle = C.c_void_p(gone._h.value)
    gone.close()
    with pytest.raises(DvError, match="closed"):
        gone.fit_flux_groups()
    assert raw(h=handle, rows=0) == -5
    # a set without rows fits nothing
    empty = eng.open_field_set(fields[:1])
    empty.keep_stamps()
    out = empty.fit_flux_groups()
    assert out["fit_scale"].shape == (0, NB) and out["fit_group"].shape == (0,)
    empty.close()


def test_a_group_of_1025_is_refused_by_name():
    """A chain of 1025 stamps that overlap their neighbours by one pixel, 600 of it placed in pass 0 and 425 in pass 1, in field 1
    of a set whose field 0 holds three stamps per pass; nothing of the chain is fitted"""
    from debvader_amd._lib import DvError

    Fbig = 1500
    net = _net("float32")
    eng = net._core.engine
    path = fgo.serpentine(1025, CS, Fbig)
    fields = np.tile(np.random.default_rng(4).normal(0, 0.05, size=(100, 100, NB)), (2, Fbig // 100, Fbig // 100, 1))
    three = np.array([(0, 0), (100, 100), (700, 40)], np.int32)
    fs = eng.open_field_set(fields)
    fs.keep_stamps()
    try:
        for p, (a, z) in enumerate([(0, 600), (600, 1025)]):
            pl = np.concatenate([three, path[a:z]]).astype(np.int32)
            fs.deblend_pass_measure(pl, pl, np.array([0, 3, 3 + z - a], np.int64), seed=90 + p)
        sums = fs.blend_sums()
        assert sums.shape == (1031, 4)
        with pytest.raises(DvError, match=r"dv_field_set_fit_flux_groups: field 1: the blend group of row 0 has 1025 galaxies, the "
                                          r"grouped fit takes at most 1024 per group"):
            fs.fit_flux_groups()
        assert _eq(fs.blend_sums(), sums)                           # the set gives the bits it gave before
    finally:
        fs.close()


# ---- 6: the class -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["reference", "cumulative"])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_the_class_with_the_grouped_fit(dtype, mode):
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

    sky = np.linspace(0.04, 0.06, NB)
    dense, res0, _ = run(blendedness=True, fit_flux=True, sky_sigma=sky)
    grouped, res1, net = run(blendedness=True, fit_flux=True, sky_sigma=sky, fit_groups=True)
    denw, res2, _ = run(fit_flux=True, fit_weights=W, return_fields=False)
    grpw, res3, _ = run(fit_flux=True, fit_weights=W, fit_groups=True, return_fields=False)
    assert dense.mse == grouped.mse == denw.mse == grpw.mse and max(len(m) for m in dense.mse) >= 2
    assert np.array_equal(grouped.get_residual_fields(), dense.get_residual_fields())
    base = B.COLUMNS + B.catalogue_columns(NB, True)
    assert all(r.dtype == np.dtype(base + ms.fit_flux_dtype(NB) + ms.fit_groups_dtype(NB)) for r in res1)
    lean = B.COLUMNS + B.catalogue_columns(NB, False)
    assert all(r.dtype == np.dtype(lean + ms.fit_flux_weighted_dtype(NB) + ms.fit_groups_dtype(NB)) for r in res3)
    # every column shared with the run without the option, from the same seed counter
    for a, b in ((res1, res0), (res3, res2)):
        for m in range(4):
            assert a[m].dtype.names[:len(b[m].dtype.names)] == b[m].dtype.names
            for k in b[m].dtype.names:
                if k != "shifts":
                    assert _eq(np.asarray(a[m][k]), np.asarray(b[m][k])), (m, k)
    # the stamps of every pass, re-derived: a plain set walks the same passes, infer_fields cuts from its working residual
    eng = net._core.engine
    passes = max(len(mm) for mm in dense.mse)
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
    sizes = []
    for m in range(4):
        if not len(res0[m]):
            assert len(res1[m]) == 0 and len(res3[m]) == 0
            continue
        s, p = np.concatenate(stamps[m]), np.concatenate(places[m])
        want = ms.fit_fluxes_groups(s, p, fields[m], catalogue=res0[m], sky_sigma=sky)
        for k in want.dtype.names:
            assert _eq(np.asarray(res1[m][k]), np.asarray(want[k])), (m, k)
        want = ms.fit_fluxes_groups(s, p, fields[m], catalogue=res0[m], weights=W[m])
        for k in want.dtype.names:
            assert _eq(np.asarray(res3[m][k]), np.asarray(want[k])), (m, k)
        # the label is an index into the field's own recarray
        g = np.asarray(res1[m]["fit_group"])
        assert (g <= np.arange(len(g))).all() and np.array_equal(g[g], g)
        sizes.append(int(np.asarray(res1[m]["fit_group_size"]).max()))
    print(f"[{dtype} {mode}] passes per field {[len(mm) for mm in dense.mse]}, galaxies {[len(r) for r in res0]}, largest group "
          f"per field {sizes}")
    assert sum(len(r) for r in res0) >= 10
