"""The GPU source detector (Context.scene_detect, csrc/detect.hip) stage by stage against its numpy restatement
(tests/detect_oracle.py), detect_objects and IterativeDeblendField end to end."""
import os

import numpy as np
import pytest

from tests import detect_oracle as do

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _ctx():
    from debvader_amd import engine as E
    return E.default_context()


def _golden():
    return np.load(os.path.join(HERE, "golden", "detect.npz"))


def _gauss(shape, cy, cx, sig, amp):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return amp * np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / sig ** 2)


def _compare(got, i, exp):
    """field i of a scene_detect result with maps against the oracle's detect() of the same field"""
    for k in ("back", "rms", "D"):
        scale = np.abs(exp[k]).max()
        np.testing.assert_allclose(got[k][i], exp[k], rtol=0, atol=1e-12 * scale, err_msg=k)
    np.testing.assert_allclose(got["globalrms"][i], exp["globalrms"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(got["labels"][i], exp["labels"])
    lo, hi = got["offsets"][i], got["offsets"][i + 1]
    assert hi - lo == len(exp["x"]), (hi - lo, len(exp["x"]))
    assert (got["field"][lo:hi] == i).all()
    np.testing.assert_array_equal(got["npix"][lo:hi], exp["npix"])
    np.testing.assert_array_equal(got["parent"][lo:hi], exp["parent"])
    for k in ("peak", "flux"):
        scale = max(np.abs(exp[k]).max(), 1e-300) if len(exp[k]) else 1.0
        np.testing.assert_allclose(got[k][lo:hi], exp[k], rtol=0, atol=1e-12 * scale, err_msg=k)
    for k in ("x", "y"):
        np.testing.assert_allclose(got[k][lo:hi], exp[k], rtol=0, atol=1e-9, err_msg=k)


def _check(field, **kw):
    got = _ctx().scene_detect(field[None], return_maps=True, **kw)
    exp = do.detect(field, **kw)
    _compare(got, 0, exp)
    return got, exp


def _blends(H, W, seed):
    rng = np.random.default_rng(seed)
    f = 100.0 + rng.normal(0, 1.0, (H, W))
    for cy, cx, s, a in ((40, 40, 2.0, 30.0), (40, 46, 2.5, 20.0), (0, 80, 2.0, 25.0), (H - 2, W - 1, 3.0, 40.0),
                         (120, 10, 1.5, 15.0), (150, 150, 4.0, 12.0), (154, 157, 2.0, 18.0), (100, 200, 2.0, 9.0)):
        f += _gauss((H, W), cy, cx, s, a)
    return f


def test_dc2_fields_stage_by_stage():
    z = _golden()
    for k in (2, 3):
        got, exp = _check(z[f"field{k}_r"].astype(np.float64))
        assert len(exp["x"]) > 30


def test_synthetic_blends_edges_and_shapes():
    got, exp = _check(_blends(200, 259, 4))                   # H != W, partial meshes, objects touching the edges
    assert (exp["npix"] > 0).all() and len(set(exp["parent"])) < len(exp["parent"])      # some components were split
    _check(_blends(200, 259, 5), nthresh=32, cont=1e-3, minarea=6, back_size=32, back_filter=5,
           filter_kernel=np.outer([1.0, 2.0, 1.0], [1.0, 3.0, 4.0, 3.0, 1.0]))
    rng = np.random.default_rng(6)
    small = rng.normal(0, 1, (40, 50)) + _gauss((40, 50), 20, 25, 2.0, 30.0)   # smaller than one mesh
    got, exp = _check(small)
    assert len(exp["x"]) == 1


def test_component_above_the_lds_budget_takes_the_global_path():
    rng = np.random.default_rng(7)
    f = rng.normal(0, 1, (256, 256)) + _gauss((256, 256), 120, 110, 15.0, 100.0) + \
        _gauss((256, 256), 126, 150, 10.0, 80.0) + _gauss((256, 256), 30, 200, 2.0, 20.0)
    got, exp = _check(f)
    assert exp["npix"].max() > 2048 and len(exp["x"]) >= 3
    big = exp["parent"][np.argmax(exp["npix"])]
    assert (exp["parent"] == big).sum() >= 2                  # the large component was deblended on global scratch


def test_bit_reproducible_and_independent_of_the_batch():
    z = _golden()
    fields = np.stack([z["field2_r"].astype(np.float64), _blends(259, 259, 8), z["field3_r"].astype(np.float64)])
    ctx = _ctx()
    a = ctx.scene_detect(fields, return_maps=True)
    b = ctx.scene_detect(fields, return_maps=True)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # one field per launch (a workspace cap that fits one field) and each field alone give the same bits
    c = ctx.scene_detect(fields, return_maps=True, workspace_bytes=12 << 20)
    for k in a:
        np.testing.assert_array_equal(a[k], c[k], err_msg=k)
    for i in range(3):
        one = ctx.scene_detect(fields[i:i + 1], return_maps=True)
        lo, hi = a["offsets"][i], a["offsets"][i + 1]
        for k in ("parent", "npix", "peak", "flux", "x", "y"):
            np.testing.assert_array_equal(one[k], a[k][lo:hi], err_msg=k)
        for k in ("back", "rms", "D", "labels"):
            np.testing.assert_array_equal(one[k][0], a[k][i], err_msg=k)
        np.testing.assert_array_equal(one["globalrms"][0], a["globalrms"][i])


def test_one_field_per_launch_gives_the_same_bytes_on_non_square_fields():
    """three 48 x 40 fields on 3 x 3 meshes of 16 px, a few sources each: the default workspace (one launch) against a
    workspace that holds exactly one field (three launches), every output"""
    import re

    from debvader_amd._lib import DvError

    rng = np.random.default_rng(21)
    fields = 10.0 + rng.normal(0, 1.0, (3, 48, 40))
    for i, srcs in enumerate((((12, 10), (30, 28), (40, 8)), ((8, 30), (24, 20)), ((20, 12), (36, 30), (10, 34)))):
        for cy, cx in srcs:
            fields[i] += _gauss((48, 40), cy, cx, 1.8, 30.0)
    ctx = _ctx()
    kw = dict(back_size=16, return_maps=True)
    a = ctx.scene_detect(fields, **kw)
    assert (np.diff(a["offsets"]) >= 2).all()
    with pytest.raises(DvError, match="workspace") as refused:
        ctx.scene_detect(fields, workspace_bytes=1, **kw)
    need = int(re.search(r"needs up to (\d+) bytes", str(refused.value)).group(1))
    b = ctx.scene_detect(fields, workspace_bytes=need, **kw)
    assert set(a) == set(b) and {"back", "rms", "D", "labels"} <= set(a)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_detect_objects_equals_the_oracle_restatement():
    from debvader_amd.detect.detection import detect_objects, detect_objects_batch

    z = _golden()
    img = np.zeros((2, 259, 259, 6))
    img[0, :, :, 2] = z["field2_r"]
    img[1, :, :, 2] = z["field3_r"]
    img[:, :, :, 0] = 5.0                                      # other bands do not matter
    for i in range(2):
        got = detect_objects(img[i:i + 1])
        np.testing.assert_array_equal(got, do.detect_objects(img[i:i + 1]))
        assert got.ndim == 2 and got.shape[1] == 2
    for i, got in enumerate(detect_objects_batch(img)):
        np.testing.assert_array_equal(got, do.detect_objects(img[i:i + 1]))
    empty = detect_objects(np.full((1, 64, 64, 6), 3.0))
    assert empty.shape == (0,)


def test_field_above_the_workspace_cap_is_refused():
    from debvader_amd._lib import DvError

    with pytest.raises(DvError, match="workspace"):
        _ctx().scene_detect(np.zeros((1, 259, 259)), workspace_bytes=1 << 20)


def _net():
    from debvader_amd.model.model import create_model_vae
    net, _, _, _ = create_model_vae((59, 59, 6), 32, [32, 64, 128, 256], [3, 3, 3, 3])
    return net


def _dc2_field(k):
    z = _golden()
    f = np.zeros((1, 259, 259, 6))
    for b in range(6):
        f[0, :, :, b] = z[f"field{k}_r"] * (0.5 + 0.1 * b)
    return f


def test_iterative_deblend_field_end_to_end():
    from debvader_amd.deblend_iterative.iterative_deblender import IterativeDeblendField

    field = _dc2_field(2)
    it = IterativeDeblendField(_net(), field)
    res = it.iterative_deblending()
    # the loop ended; one mse per pass; the first pass deblended what the detector found on the field
    first = do.detect_objects(field)
    assert it.nb_of_detected_objects[0] == len(first)
    assert len(it.mse) >= 2
    assert res is not None and len(res) >= it.nb_of_deblended_galaxies[0]
    n0 = it.nb_of_deblended_galaxies[0]
    idx0 = np.asarray(res["list_idx"][:n0])                   # detections of the first pass whose cutout fits the field
    assert (np.diff(idx0) > 0).all() and idx0[-1] < len(first)
    assert len(res) >= sum(it.nb_of_deblended_galaxies) and len(it.mse) >= len(it.nb_of_deblended_galaxies)
    if len(it.nb_of_deblended_galaxies) > 1:                  # later passes are offset by the galaxies before them
        assert res["list_idx"][n0] >= n0
    assert np.isfinite(it.mse).all()
    # positions fitted in every pass
    it2 = IterativeDeblendField(_net(), field)
    res2 = it2.iterative_deblending(optimise_positions=True)
    sh = np.array([np.asarray(s, np.float64) for s in res2["shifts"]])
    assert sh.dtype == np.float64 and sh.shape == (len(res2), 2) and (np.abs(sh) <= 3.0).all()
    assert isinstance(res2["shifts"][0], np.ndarray) and res2["shifts"][0].dtype == np.float64


def test_iterative_deblend_field_with_nothing_to_detect():
    from debvader_amd.deblend_iterative.iterative_deblender import IterativeDeblendField

    it = IterativeDeblendField(None, np.full((1, 128, 128, 6), 2.0))
    assert it.iterative_deblending() is None
    assert it.mse == [0.0]
