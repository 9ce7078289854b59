"""The GPU detector's segmentation and deblender (cc_merge / cc_flatten / cc_compact / deblend_kernel of csrc/detect.hip) on
the painted fields of tests/detect_shapes.py: fields in which back == 0 and D == data bit for bit, so that the union-find,
the column guards, the level loop, the decision rule, the renumbering, the tie rules and the catalogue's order meet exactly
the integers that were painted.  tests/test_detect_shapes_host.py asserts the premises (P1 - P5) on the CPU; here every
case goes through Context.scene_detect(return_maps=True) and is compared with the numpy restatement under the rules of
tests/test_gpu_detect.py and tests/test_gpu_detect_weighted.py (back is 0, so its bound 1e-12 max|back| is equality)."""
import re

import numpy as np
import pytest

from tests import detect_oracle as do
from tests import detect_shapes as ds
from tests.test_gpu_detect import _compare as _compare_unweighted
from tests.test_gpu_detect_weighted import _compare as _compare_weighted
from tests.test_gpu_detect_weighted import _same_bits

pytestmark = pytest.mark.gpu

CASES = ("row_wrap", "diagonals", "serpentine", "spiral", "half_serpentine", "lattice", "lattice_minarea2", "comb",
         "nested_mesas", "insignificant", "plateaus")
CAT = ("field", "parent", "npix", "peak", "flux", "x", "y")
MAPS = ("back", "rms", "D", "labels")


def _ctx():
    from debvader_amd import engine as E
    return E.default_context()


def _ones(a):
    return np.ones(a.shape)


def _exact_maps(got, i, data):
    """what the premises promise of the device as well: no background, and D the painted field"""
    assert (got["back"][i] == 0.0).all()
    np.testing.assert_array_equal(got["D"][i], data)


@pytest.mark.parametrize("name", CASES)
def test_weighted_path(name):
    data, exp, _, kw = ds.oracle(name)
    got = _ctx().scene_detect(data[None], weights=_ones(data)[None], return_maps=True, **kw)
    _compare_weighted(got, 0, exp)
    _exact_maps(got, 0, data)


@pytest.mark.parametrize("name", [n for n in CASES if n in ds.UNWEIGHTED])
def test_unweighted_path(name):
    data, exp, _, kw = ds.oracle(name, "unweighted")
    got = _ctx().scene_detect(data[None], return_maps=True, **kw)
    _compare_unweighted(got, 0, exp)
    _exact_maps(got, 0, data)


def test_every_case_has_its_unweighted_twin_or_a_reason():
    """the cases left out of test_unweighted_path are those whose globalrms is 0 (tests/test_detect_shapes_host.py)"""
    assert set(CASES) - set(ds.UNWEIGHTED) == {"row_wrap", "diagonals", "insignificant"}


@pytest.mark.parametrize("name", CASES)
def test_as_one_field_of_a_batch(name):
    """the case between two other painted fields, under its own settings: its seams are par + f * HW on both sides"""
    data, exp, _, kw = ds.oracle(name)
    fields = np.stack([ds.CASES["plateaus"]()[0], data, ds.CASES["diagonals"]()[0]])
    got = _ctx().scene_detect(fields, weights=_ones(fields), return_maps=True, **kw)
    _compare_weighted(got, 1, exp)
    _exact_maps(got, 1, data)
    assert got["offsets"][1] > 0 and got["offsets"][3] == len(got["x"])
    if name in ds.UNWEIGHTED:
        data, exp, _, kw = ds.oracle(name, "unweighted")
        # the neighbours are the case itself: every field of an unweighted batch has its own threshold
        got = _ctx().scene_detect(np.stack([data, data[::-1], data]), return_maps=True, **kw)
        for i in (0, 2):
            _compare_unweighted(got, i, exp)
            _exact_maps(got, i, data)


def _need(msg):
    m = re.search(r"needs up to (\d+) bytes", msg)
    assert m, msg
    return int(m.group(1))


def test_batch_seams():
    """more than a thousand components next to none, a painted last row before a painted first row, then the comb: every
    field against the oracle, against itself alone and against a workspace that admits one field per launch"""
    from debvader_amd._lib import DvError

    fields = np.stack([ds.oracle(n)[0] for n in ds.BATCH])
    kw = ds.oracle(ds.BATCH[0])[3]
    w = _ones(fields)
    ctx = _ctx()
    a = ctx.scene_detect(fields, weights=w, return_maps=True, **kw)
    for i, name in enumerate(ds.BATCH):
        exp = ds.oracle(name)[1]
        _compare_weighted(a, i, exp)
        _exact_maps(a, i, fields[i])
        one = ctx.scene_detect(fields[i:i + 1], weights=w[i:i + 1], return_maps=True, **kw)
        lo, hi = a["offsets"][i], a["offsets"][i + 1]
        assert hi - lo == len(one["x"]) == len(exp["x"])
        for k in CAT[1:]:
            np.testing.assert_array_equal(one[k], a[k][lo:hi], err_msg=k)
        for k in MAPS:
            np.testing.assert_array_equal(one[k][0], a[k][i], err_msg=k)
        assert one["globalrms"][0] == a["globalrms"][i]
    assert np.diff(a["offsets"]).tolist() == [1426, 0, 1, 1, 25]
    with pytest.raises(DvError, match="workspace") as refused:
        ctx.scene_detect(fields, weights=w, return_maps=True, workspace_bytes=1, **kw)
    need = _need(str(refused.value))                   # what one field needs: a cap that admits one field per launch
    _same_bits(a, ctx.scene_detect(fields, weights=w, return_maps=True, workspace_bytes=need, **kw))


def test_band_gather():
    """detect_objects_batch on (2, H, W, 6): band 2 holds the nested mesas in one field and the comb in the other, every
    other band another painted field"""
    from debvader_amd.detect.detection import detect_objects_batch

    img = np.empty((2, ds.H, ds.W, 6))
    decoys = [ds.CASES[n]()[0] for n in ds.DECOYS]
    for f in range(2):
        for j, b in enumerate((0, 1, 3, 4, 5)):
            img[f, :, :, b] = decoys[(j + 2 * f) % len(decoys)]
        img[f, :, :, 2] = ds.oracle(ds.BANDS[f], "unweighted")[0]
    got = detect_objects_batch(img, filter_kernel=ds.K1)
    assert [len(g) for g in got] == [4, 25]
    for f in range(2):
        np.testing.assert_array_equal(got[f], do.detect_objects(img[f:f + 1], filter_kernel=ds.K1))
