"""The painted fields of tests/detect_shapes.py against their own premises, on the CPU: what tests/test_gpu_detect_shapes.py
compares the GPU detector with is only exact, and only aimed where it claims, if P1 - P5 hold for the numpy restatement
alone.  A premise that fails is a fault of the painted input, never a reason to skip the case."""
import numpy as np
import pytest

from tests import detect_shapes as ds


@pytest.mark.parametrize("name", list(ds.CASES))
def test_premises_on_the_weighted_path(name):
    data, exp, details, kw = ds.oracle(name)
    assert data.shape == (ds.H, ds.W) and ds.H != ds.W and all(n % 16 and n % 64 for n in data.shape)
    assert exp["bad_meshes"] == 0 and ds.threshold(exp, kw) == 0.5
    painted = data[data != 0]
    assert (painted == np.round(painted)).all() and (painted >= 1).all() and (painted <= 7).all()
    ds.check_premises(data, exp, details, kw)
    ds.check_facts(data, exp, details, ds.CASES[name]()[2])


@pytest.mark.parametrize("name", list(ds.CASES))
def test_labels_equal_scipy_alone(name):
    data, exp, _, kw = ds.oracle(name)
    np.testing.assert_array_equal(exp["labels"], ds.scipy_labels(data, 0.5, kw["minarea"] if "minarea" in kw else 4))
    if name in ds.UNWEIGHTED:
        data, exp, _, kw = ds.oracle(name, "unweighted")
        np.testing.assert_array_equal(exp["labels"],
                                      ds.scipy_labels(data, 1.5 * exp["globalrms"], kw["minarea"] if "minarea" in kw else 4))


@pytest.mark.parametrize("name", list(ds.CASES))
def test_unweighted_twin(name):
    """UNWEIGHTED is the list of the cases whose twin sees the painted integers: 0 < 1.5 globalrms < 0.9 min(painted);
    for those P1 - P5 hold on the unweighted path as well.  (In the other cases the painted pixels are too few to survive
    the meshes' clipping and globalrms is 0.)"""
    if name not in ds.UNWEIGHTED:
        data, _, _ = ds.CASES[name]()
        bk = ds.do.background(data)
        assert not ds.unweighted_premise(data, bk) and bk["globalrms"] == 0.0
        return
    data, exp, details, kw = ds.oracle(name, "unweighted")
    assert ds.unweighted_premise(data, exp)
    assert 0.0 < 1.5 * exp["globalrms"] < 0.9 * data[data > 0].min()
    ds.check_premises(data, exp, details, kw)
    ds.check_facts(data, exp, details, ds.CASES[name]()[2])


def test_the_batch_and_the_bands_are_what_the_gpu_tests_take_them_for():
    kws = [ds.oracle(name)[3] for name in ds.BATCH]
    assert all(k["minarea"] == 1 and k.keys() == kws[0].keys() for k in kws)          # one call: one set of settings
    ncomp = [len(ds.oracle(name)[2]) for name in ds.BATCH]
    assert ncomp[0] > 1000 and ncomp[1] == 0 and ncomp[2] == ncomp[3] == 1 and ncomp[4] == 1
    assert not set(ds.BATCH[1:4]) & set(ds.UNWEIGHTED)            # the batch runs on the weighted path alone
    # the band-gather case is unweighted with the default settings; its decoys differ from band 2 and from each other
    assert set(ds.BANDS) <= set(ds.UNWEIGHTED) and all(ds.CASES[n]()[1] == {} for n in ds.BANDS)
    planes = [ds.CASES[n]()[0] for n in ds.BANDS + ds.DECOYS]
    assert all(not np.array_equal(a, b) for i, a in enumerate(planes) for b in planes[:i])
