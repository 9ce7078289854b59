"""The flux fit by blend groups without a GPU: the definition on the numpy restatement of
tests/fit_flux_groups_oracle.py - the groups of a scene by hand, relabelling, long chains, the grouped solution against the dense
restatement on the whole field - and the host layer (measurement.fit_groups_records / fit_fluxes_groups,
DeblendFieldBatch.deblend_fields(fit_groups=True), the engine wrappers and the ctypes signatures) over the stand-ins of
tests/stub_fit_flux_groups_engine.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import fit_flux_groups_oracle as go
from tests import fit_flux_oracle as fo
from tests import fit_flux_weighted_oracle as fw
from tests.stub_fit_flux_groups_engine import CS, GKEYS, KEYS, NB, WKEYS, Net, OracleContext, stub_fit_groups
from tests.stub_fit_flux_weighted_engine import stub_fit_flux_weighted
from tests.stub_measure_engine import stub_catalogue
from tests.test_fit_flux_host import CS31, M1, M2, O1, O2, _c_types, _paste, _stamp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FH = 200
NAMES = ["lone a", "pair a", "triple a", "lone b", "pair b", "triple b", "outside", "triple c", "duplicate"]
PLACES = np.array([[5, 5], [60, 5], [100, 60], [150, 150], [60, 25], [115, 80], [-40, 10], [130, 100], [115, 80]])
GROUP, SIZE = [0, 1, 2, 3, 1, 2, 6, 2, 2], [1, 2, 4, 1, 2, 4, 1, 4, 4]


def _hand():
    """The kinds of galaxy of the scene of section 7l in one 200-pixel field, far enough apart that the rectangles say what the
    names say: two lone galaxies, a pair, a chain of three (a - b - c: a and c touch only through b), a stamp wholly outside, and
    an exact duplicate of "triple b" behind them; the rows of the pair and the triple are not contiguous"""
    mk = lambda i: _stamp(M1 if i % 2 else M2, O1 if i % 3 else O2, amp=1.0 + 0.1 * i)     # noqa: E731
    P = np.stack([mk(i) for i in range(len(NAMES))])
    P[8] = P[5]
    amps = np.linspace(0.8, 1.25, len(NAMES))
    D = _paste(FH, P, PLACES, amps) + np.random.default_rng(2).normal(0.0, 0.02, size=(FH, FH, 3))
    return P, PLACES, D


def test_the_groups_of_a_scene_by_hand():
    group, size = go.groups(PLACES, [0, len(PLACES)], CS31, FH)
    assert group.tolist() == GROUP and size.tolist() == SIZE and group.dtype == size.dtype == np.int32
    A = go.adjacency(PLACES, CS31, FH)
    assert not A[6].any() and not A[:, 6].any()                     # wholly outside: adjacent to nothing, itself included
    assert A[2, 5] and A[5, 7] and not A[2, 7] and A[5, 8] and A.diagonal().sum() == 8
    # two fields: the labels count from the field's first row
    group2, size2 = go.groups(np.concatenate([PLACES[:4], PLACES]), [0, 4, 4 + len(PLACES)], CS31, FH)
    assert group2.tolist() == [0, 1, 2, 3] + GROUP and size2.tolist() == [1, 1, 1, 1] + SIZE
    # the lists the fit works from: (i, j <= i) sorted by i then j, ascending adjacency lists, the diagonal included
    pairs, ptr, adj = go.lists(PLACES, [0, len(PLACES)], CS31, FH)
    assert pairs.tolist() == [[0, 0], [1, 1], [2, 2], [3, 3], [4, 1], [4, 4], [5, 2], [5, 5], [7, 5], [7, 7], [8, 2], [8, 5], [8, 7], [8, 8]]
    assert np.diff(ptr).tolist() == [1, 2, 3, 1, 2, 4, 0, 3, 4] and adj[ptr[5]:ptr[6]].tolist() == [2, 5, 7, 8]
    order, gptr, gfield = go.group_order(group, [0, len(PLACES)])
    assert order.tolist() == [0, 1, 4, 2, 5, 7, 8, 3, 6] and gptr.tolist() == [0, 1, 3, 7, 8, 9] and gfield.tolist() == [0] * 5


def test_relabelling_permutes_the_sizes_and_keeps_the_partition():
    rng = np.random.default_rng(8)
    places = rng.integers(-20, 290, size=(120, 2))
    group, size = go.groups(places, [0, 120], CS31, 300)
    assert 1 < len(np.unique(group)) < 120
    for _ in range(3):
        perm = rng.permutation(120)
        g2, s2 = go.groups(places[perm], [0, 120], CS31, 300)
        assert np.array_equal(s2, size[perm])
        same = group[perm][:, None] == group[perm][None, :]
        assert np.array_equal(g2[:, None] == g2[None, :], same)
        assert all(g2[i] == np.nonzero(same[i])[0].min() for i in range(120))    # the label is the smallest row of the group


def test_long_chains_and_a_grid():
    cs, n = 9, 1025
    chain = go.serpentine(n, cs, 400)
    A = go.adjacency(chain, cs, 400)
    assert all(A[i, i + 1] for i in range(n - 1))
    step = chain[1:] - chain[:-1]
    assert (np.abs(step).sum(axis=1) == cs - 1).all()                # consecutive stamps share one row or column of pixels
    group, size = go.groups(chain, [0, n], cs, 400)
    assert (group == 0).all() and (size == n).all()
    perm = np.random.default_rng(1).permutation(n)
    group, size = go.groups(chain[perm], [0, n], cs, 400)
    assert (group == 0).all() and (size == n).all()
    cells = np.arange(n)
    grid = np.stack([(cells // 41) * cs, (cells % 41) * cs], axis=1)
    group, size = go.groups(grid, [0, n], cs, 400)
    assert group.tolist() == cells.tolist() and (size == 1).all()


@pytest.mark.parametrize("weighted", [False, True])
def test_the_grouped_solution_is_the_dense_one(weighted):
    """The bounds of tests/test_fit_flux_host.py's closed forms: 1e-11 on the amplitudes, 1e-12 relative on the variances"""
    P, places, D = _hand()
    fp = [0, len(P)]
    if weighted:
        W = np.random.default_rng(4).uniform(0.5, 2.0, size=D.shape)
        W[60:70, 20:40] = 0.0
        got, per_group = go.fit_flux_groups(P, places, fp, D[None], W[None])
        want, _ = fw.fit_flux(P, places, fp, D[None], W[None])
    else:
        got, per_group = go.fit_flux_groups(P, places, fp, D[None])
        want, _ = fo.fit_flux(P, places, fp, D[None])
    assert len(per_group) == 5 and got["fit_group"].tolist() == GROUP and got["fit_group_size"].tolist() == SIZE
    assert np.array_equal(got["fit_status"], want["fit_status"])
    assert got["fit_status"].tolist() == [[0] * 3] * 6 + [[4] * 3] + [[0] * 3] + [[5] * 3]
    for k in ("fit_gram", "fit_proj") + (("fit_npix",) if weighted else ()):
        assert np.array_equal(got[k], want[k]), k                    # the same sums over the same pixels
    ok = want["fit_status"] == 0
    assert np.array_equal(np.isnan(got["fit_scale"]), np.isnan(want["fit_scale"]))
    assert np.array_equal(np.isnan(got["fit_var"]), np.isnan(want["fit_var"]))
    assert np.abs(got["fit_scale"][ok] - want["fit_scale"][ok]).max() < 1e-11
    assert (np.abs(got["fit_var"][ok] - want["fit_var"][ok]) <= 1e-12 * want["fit_var"][ok]).all()
    assert (got["fit_scale"][8] == 1.0).all()                        # the dropped duplicate keeps the network's amplitude
    if weighted:
        c = want["fit_status"] != 4
        assert np.abs(got["fit_chi2"][c] - want["fit_chi2"][c]).max() <= 1e-9 * want["chi2_yard"][c].max()
        assert np.isnan(got["fit_chi2"][6]).all()


# ---- the host layer -----------------------------------------------------------------------------------------------------------
def test_columns_and_records():
    from debvader_amd.measure import measurement as ms

    assert ms.fit_groups_dtype(3) == [("fit_group", "<i4"), ("fit_group_size", "<i4")] == ms.fit_groups_dtype(6)
    rec = ms.fit_groups_records([0, 0, 2], [2, 2, 1])
    assert rec.dtype == np.dtype(ms.fit_groups_dtype(3)) and rec["fit_group"].tolist() == [0, 0, 2]
    assert rec["fit_group_size"].tolist() == [2, 2, 1]
    for bad in (([0, 1], [1]), ([[0]], [[1]])):
        with pytest.raises(ValueError, match="expected fit_group and fit_group_size"):
            ms.fit_groups_records(*bad)
    p = inspect.signature(ms.fit_fluxes_groups).parameters
    assert list(p) == ["stamps_mean", "places", "data_fields", "field_ptr", "catalogue", "sky_sigma", "weights", "min_pivot", "ctx"]
    assert p["weights"].default is None and p["min_pivot"].default == 1e-8


def test_fit_fluxes_groups_over_the_restatement():
    from debvader_amd.measure import measurement as ms

    P, places, D = _hand()
    ctx = OracleContext()
    rec = ms.fit_fluxes_groups(P, places, D, ctx=ctx)
    assert rec.dtype == np.dtype(ms.fit_flux_dtype(3) + ms.fit_groups_dtype(3))
    assert ctx.calls[-1]["fit_flux_groups"] == 9 and ctx.calls[-1]["weights"] is None and ctx.calls[-1]["field_ptr"] == [0, 9]
    assert rec["fit_group"].tolist() == GROUP and rec["fit_group_size"].tolist() == SIZE
    want, _ = go.fit_flux_groups(P, places, [0, 9], D[None])
    flux = P.sum(axis=(1, 2), dtype=np.float64)
    plain = ms.fit_flux_records(*(want[k] for k in KEYS), flux)
    for k in plain.dtype.names:
        assert np.array_equal(rec[k], plain[k], equal_nan=True), k
    assert np.isnan(rec["fit_scale_err"]).all()
    # sky_sigma: per band or per field and band, the error columns scale with it; a wrong shape is refused before the context
    sig = np.array([0.1, 0.2, 0.3])
    rec = ms.fit_fluxes_groups(P, places, D, sky_sigma=sig, ctx=ctx)
    assert np.array_equal(rec["fit_scale_err"], sig * np.sqrt(want["fit_var"]), equal_nan=True)
    two = ms.fit_fluxes_groups(np.concatenate([P, P]), np.concatenate([places, places]), np.stack([D, D]), field_ptr=[0, 9, 18],
                               sky_sigma=np.stack([sig, 2 * sig]), ctx=ctx)
    assert np.array_equal(two["fit_scale_err"][9:], 2 * rec["fit_scale_err"], equal_nan=True)
    assert two["fit_group"].tolist() == GROUP + GROUP
    n = len(ctx.calls)
    with pytest.raises(ValueError, match="sky_sigma"):
        ms.fit_fluxes_groups(P, places, D, sky_sigma=np.ones(2), ctx=ctx)
    # weights: the weighted columns, then the groups; the noise is given once; the shape is checked before the context
    W = np.random.default_rng(4).uniform(0.5, 2.0, size=D.shape)
    with pytest.raises(ValueError, match="weights already carry the noise"):
        ms.fit_fluxes_groups(P, places, D, weights=W, sky_sigma=sig, ctx=ctx)
    with pytest.raises(ValueError, match="expected weight fields of the shape of the data fields"):
        ms.fit_fluxes_groups(P, places, D, weights=W[:50], ctx=ctx)
    with pytest.raises(ValueError, match="lacks the column flux"):
        ms.fit_fluxes_groups(P, places, D, catalogue=np.recarray((9,), dtype=[("x", "<f8")]), ctx=ctx)
    assert len(ctx.calls) == n
    rec = ms.fit_fluxes_groups(P, places, D, weights=W, ctx=ctx)
    assert rec.dtype == np.dtype(ms.fit_flux_weighted_dtype(3) + ms.fit_groups_dtype(3))
    assert ctx.calls[-1]["weights"] == (1, FH, FH, 3)
    wantw, _ = go.fit_flux_groups(P, places, [0, 9], D[None], W[None])
    assert np.array_equal(rec["fit_chi2"], wantw["fit_chi2"], equal_nan=True) and np.array_equal(rec["fit_npix"], wantw["fit_npix"])
    assert np.array_equal(rec["fit_scale_err"], np.sqrt(wantw["fit_var"]), equal_nan=True)


F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[100.0, 0.0], [-3.0, 11.0]]), np.array([[0.0, 40.0]])]


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(4, F, F, NB)), CS, NB)


def _engine_calls(net):
    return [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_deblend_fields_appends_the_group_columns():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch
    from debvader_amd.measure import measurement as ms

    sig = inspect.signature(DeblendFieldBatch.deblend_fields).parameters
    assert sig["fit_groups"].default is False and sig["fit_groups"].kind is inspect.Parameter.KEYWORD_ONLY
    assert DeblendFieldBatch.fit_groups_columns(NB) == ms.fit_groups_dtype(NB)
    net, b = _batch()
    W = np.random.default_rng(5).uniform(0.5, 2.0, size=(4, F, F, NB))
    base = DeblendFieldBatch.ON_DEVICE_COLUMNS + DeblendFieldBatch.measure_columns(NB)
    g = stub_fit_groups(3)
    for rf in (True, False):
        # unweighted, with sky_sigma: the columns of fit_flux, then the two of the groups
        res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True, fit_groups=True, sky_sigma=np.ones(NB),
                               return_fields=rf)
        call = _engine_calls(net)[-1]
        assert call[0] == "infer_fields_measure_fit_groups" and call[2] is rf and call[3] is not None and call[4] is None
        want = np.dtype(base + DeblendFieldBatch.fit_flux_columns(NB) + DeblendFieldBatch.fit_groups_columns(NB))
        assert [len(r) for r in res] == [2, 0, 1, 0] and all(r.dtype == want for r in res)
        assert res[0].dtype.names[-2:] == GKEYS
        for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
            assert res[m]["fit_group"][k] == g["fit_group"][i] and res[m]["fit_group_size"][k] == g["fit_group_size"][i]
        assert np.isfinite(res[0]["fit_scale_err"][0]).all()
        # weighted: fit_chi2 and fit_npix stand between them
        res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True, fit_groups=True, fit_weights=W, return_fields=rf)
        call = _engine_calls(net)[-1]
        assert call[0] == "infer_fields_measure_fit_groups" and np.array_equal(call[4], W)
        want = np.dtype(base + DeblendFieldBatch.fit_flux_weighted_columns(NB) + DeblendFieldBatch.fit_groups_columns(NB))
        assert all(r.dtype == want for r in res)
        f, c = stub_fit_flux_weighted(3, NB), stub_catalogue(3, NB)
        cat = ms.fit_flux_records(*(f[k] for k in KEYS), c["flux"], fit_chi2=f["fit_chi2"], fit_npix=f["fit_npix"])
        for i, (m, k) in enumerate([(0, 0), (0, 1), (2, 0)]):
            for n in cat.dtype.names:
                assert np.array_equal(res[m][n][k], cat[n][i], equal_nan=True), n
    # without fit_groups the call and the columns are those of before
    res = b.deblend_fields(DIST, on_device=True, measure=True, fit_flux=True)
    assert _engine_calls(net)[-1][0] == "infer_fields_measure_fit" and "fit_group" not in res[0].dtype.names


def test_deblend_fields_refuses_fit_groups_combinations():
    net, b = _batch()
    W = np.ones((4, F, F, NB))
    on = dict(on_device=True, measure=True)
    not_yet = "fit_groups=True cannot be combined with fit_sky or fit_nonneg: those two are not built for the grouped fit yet"
    for kw, match in ((dict(fit_groups=True, **on), "fit_groups=True needs fit_flux=True"),
                      (dict(fit_groups=True), "fit_groups=True needs fit_flux=True"),
                      (dict(fit_groups=True, fit_weights=W, **on), "needs fit_flux=True"),
                      (dict(fit_groups=True, fit_flux=True), "fit_flux=True needs measure=True and on_device=True"),
                      (dict(fit_groups=True, fit_flux=True, fit_sky=0, **on), not_yet),
                      (dict(fit_groups=True, fit_flux=True, fit_sky=1, fit_weights=W, **on), not_yet),
                      (dict(fit_groups=True, fit_flux=True, fit_nonneg=True, **on), not_yet),
                      (dict(fit_groups=True, fit_flux=True, fit_nonneg=True, fit_sky=0, **on), not_yet),
                      (dict(fit_groups=True, fit_flux=True, psf=np.ones((21, 21)), **on), "fit_flux=True cannot be combined with psf"),
                      (dict(fit_groups=True, fit_flux=True, blendedness=True, **on), "fit_flux=True cannot be combined with blendedness"),
                      (dict(fit_groups=True, fit_flux=True, optimise_positions=True, **on),
                       "fit_flux=True cannot be combined with optimise_positions"),
                      (dict(fit_groups=True, fit_flux=True, fit_weights=W, sky_sigma=np.ones(NB), **on), "weights already carry the noise"),
                      (dict(fit_groups=True, fit_flux=True, fit_weights=W[:3], **on),
                       "expected weight fields of the shape of the data fields"),
                      (dict(fit_groups=True, fit_flux=True, sky_sigma=np.ones(NB + 1), **on), "sky_sigma")):
        with pytest.raises(ValueError, match=match):
            b.deblend_fields(DIST, **kw)
    assert not _engine_calls(net) and net._core.seed_counter == 7


def test_engine_wrappers_refuse_before_the_library():
    from debvader_amd import engine as E

    P, pl, D = np.zeros((2, 31, 31, 3), np.float32), np.zeros((2, 2), np.int32), np.zeros((1, 40, 40, 3))
    call = lambda *a, **kw: E.Context.scene_fit_flux_groups(object(), *a, **kw)     # noqa: E731
    for bad in (np.zeros((1, 40, 40, 2)), np.zeros((2, 40, 40, 3)), 2.0):
        with pytest.raises(ValueError, match="expected weight fields of the shape of the data fields"):
            call(P, pl, D, weight_fields=bad)
    with pytest.raises(ValueError, match="min_pivot"):
        call(P, pl, D, min_pivot=0.0)
    with pytest.raises(ValueError, match="scratch_bytes"):
        call(P, pl, D, scratch_bytes=0)
    with pytest.raises(ValueError, match="expected square stamps"):
        call(P[:, :30], pl, D)
    with pytest.raises(ValueError, match="expected data fields"):
        call(P, pl, D[..., :2])
    with pytest.raises(ValueError, match="field_ptr is needed with 2 fields"):
        call(P, pl, np.zeros((2, 40, 40, 3)))
    # an empty call returns without the library
    empty = call(P[:0], pl[:0], D)
    assert list(empty) == list(KEYS + GKEYS) and empty["fit_group"].shape == (0,) and empty["fit_group"].dtype == np.int32
    empty = call(P[:0], pl[:0], D, weight_fields=np.ones((40, 40, 3)))
    assert list(empty) == list(WKEYS + GKEYS)
    p = inspect.signature(E.Context.scene_fit_flux_groups).parameters
    assert list(p)[1:] == list(inspect.signature(E.Context.scene_fit_flux).parameters)[1:]
    fields = np.zeros((2, 81, 81, 6))
    for kw, match in ((dict(places=None), "places are needed"),
                      (dict(places=None, return_fields=False), "places are needed"),
                      (dict(places=[[0, 0]], weight_fields=fields[:1]), "expected weight fields of the shape of the data fields"),
                      (dict(places=[[0, 0]], min_pivot=2.0), "min_pivot"),
                      (dict(places=[[0, 0]], band=7), "band")):
        places = kw.pop("places")
        with pytest.raises(ValueError, match=match):
            E.Engine.infer_fields_measure_fit_groups(object(), fields, [[0, 0]], [0, 1, 1], places, **kw)


def test_header_binding_and_library_agree_on_the_grouped_entry_points():
    from debvader_amd import _lib

    header = open(os.path.join(ROOT, "include", "debvader_hip.h")).read()
    ctype = {"dv_model*": C.c_void_p, "dv_ctx*": C.c_void_p, "double*": C.POINTER(C.c_double), "float*": C.POINTER(C.c_float),
             "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64), "int32_t": C.c_int32, "int64_t": C.c_int64,
             "uint64_t": C.c_uint64, "double": C.c_double, "dv_measure_params*": C.POINTER(_lib.DvMeasureParams),
             "dv_fit_flux_params*": C.POINTER(_lib.DvFitFluxParams)}
    for name, nargs in (("dv_scene_fit_flux_groups", 21), ("dv_infer_fields_measure_fit_groups", 31), ("dv_scene_fit_groups", 16)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/debvader_hip.h"
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)         # bound: the library exports it
        restype, argtypes = _lib.SIGNATURES[name]
        want = [ctype[t] for t in _c_types(m.group(1))]
        assert restype is C.c_int and len(argtypes) == len(want) == nargs
        for i, (a, w) in enumerate(zip(argtypes, want)):
            assert a is w, (name, i, a, w)
        assert getattr(_lib.lib, name).argtypes == argtypes
    # the unweighted scene call's arguments up to the params, the weights, the seven outputs of the weighted call, the two new
    sg, sw = _lib.SIGNATURES["dv_scene_fit_flux_groups"][1], _lib.SIGNATURES["dv_scene_fit_flux_weighted"][1]
    su = _lib.SIGNATURES["dv_scene_fit_flux"][1]
    assert sg[:11] == su[:11] and sg[11] is C.POINTER(C.c_double) and sg[12:19] == sw[12:] and sg[19:] == [C.POINTER(C.c_int32)] * 2
    # the weighted pipeline call's arguments, then the two new outputs
    pg, pw = _lib.SIGNATURES["dv_infer_fields_measure_fit_groups"][1], _lib.SIGNATURES["dv_infer_fields_measure_fit_weighted"][1]
    assert pg[:29] == pw and pg[29:] == [C.POINTER(C.c_int32)] * 2
    # the existing entry points keep their signatures, the limit its value, and the surface its rule
    assert len(su) == 16 and len(sw) == 19 and len(pw) == 29 and re.search(r"#define DV_FIT_MAX_N 1024\b", header)
    exports = open(os.path.join(ROOT, "debvader_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*dv_\*;", exports) and re.search(r"local:\s*\*;", exports)
    kernel = open(os.path.join(ROOT, "debvader_amd", "csrc", "fitflux.hip")).read()
    for k in ("fitgroups_count_kernel", "fitgroups_scan_kernel", "fitgroups_fill_kernel", "fitgroups_label_kernel",
              "template <bool WEIGHTED, int Q = 0, bool GROUPED = false>", "template <int Q, bool GROUPED = false>"):
        assert k in kernel, k
    assert "getenv" not in kernel
    engine = open(os.path.join(ROOT, "debvader_amd", "csrc", "engine.hip")).read()
    assert "launch_fit_flux_groups(" in engine and "getenv(\"DV_FIT" not in engine
