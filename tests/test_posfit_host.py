"""CPU checks of the position fit's host side: the public names, argument checks that fail before the GPU is touched, the
C-ABI entry point and the fixture's consistency with the reference's objective."""
import inspect
import os

import numpy as np
import pandas as pd
import pytest
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))


def test_reference_name_and_signature():
    from debvader_amd.deblend_cutout import optimization as O

    params = list(inspect.signature(O.position_optimization).parameters)
    assert params == ["field_image", "output_image_mean_padded", "galaxy_distance_to_center"]
    params = list(inspect.signature(O.position_optimization_batch).parameters)
    assert params[:4] == ["field_image", "stamps", "distances", "bound"]
    assert inspect.signature(O.position_optimization_batch).parameters["bound"].default == 3.0


def test_entry_point_is_bound():
    from debvader_amd import _lib

    assert "dv_scene_fit_shifts" in _lib.SIGNATURES
    assert hasattr(_lib.lib, "dv_scene_fit_shifts")


def test_band_and_shape_checks_fail_before_the_gpu():
    from debvader_amd.deblend_cutout.optimization import position_optimization, position_optimization_batch

    with pytest.raises(ValueError, match="band"):
        position_optimization_batch(np.zeros((41, 41, 2)), np.zeros((1, 11, 11, 2)), [[0, 0]])
    with pytest.raises(ValueError, match="band"):
        position_optimization(np.zeros((1, 41, 41, 1)), np.zeros((41, 41, 1)), [0, 0])
    with pytest.raises(ValueError, match="square field"):
        position_optimization_batch(np.zeros((41, 40, 3)), np.zeros((1, 11, 11, 3)), [[0, 0]])
    with pytest.raises(ValueError, match="distances"):
        position_optimization_batch(np.zeros((41, 41, 3)), np.zeros((2, 11, 11, 3)), [[0, 0]])


def test_deblend_field_points_to_optimise_positions():
    from debvader_amd.deblend.field_deblender import DeblendField

    db = DeblendField(None, np.zeros((1, 81, 81, 6)))
    with pytest.raises(NotImplementedError, match=r"optimise_positions\(\)"):
        db.deblend_field([[0, 0]], optimise_positions=True)
    with pytest.raises(ValueError, match="deblend_field"):
        db.optimise_positions()
    # the recarray of an on-device pass has no stamps
    rec = pd.DataFrame({"list_idx": [0], "shifts": [np.array([0, 0])], "galaxy_distances_to_center_x": [0.0],
                        "galaxy_distances_to_center_y": [0.0], "mse_center": [0.1],
                        "passed_cuts": [True]}).to_records(index=False)
    with pytest.raises(ValueError, match="output_images_mean"):
        db.optimise_positions(rec)


def _objective(field_r, stamp_r, d, s):
    F, cs = field_r.shape[0], stamp_r.shape[0]
    po = int((F - cs) / 2)
    pad = np.zeros((F, F))
    pad[po:po + cs, po:po + cs] = stamp_r
    net = scipy.ndimage.shift(pad, shift=(d[0], d[1]))
    return np.square(field_r - scipy.ndimage.shift(net, shift=(s[0], s[1]))).mean()


def test_fixture_objective_is_the_reference_formula():
    z = np.load(os.path.join(HERE, "golden", "posfit.npz"))
    assert len(z["real_dist"]) >= 5 and list(z["syn_names"]) == ["frac", "edge", "bound"]
    assert z["syn_dist"][0][0] != np.floor(z["syn_dist"][0][0])          # a fractional distance
    assert abs(z["syn_shift"][2][0] - 3.0) < 1e-5                           # the bound case ends on the bound
    for kind in ("real", "syn"):
        for st, d, s, j in zip(z[f"{kind}_stamps_r"], z[f"{kind}_dist"], z[f"{kind}_shift"], z[f"{kind}_objective"]):
            assert np.abs(s).max() <= 3.0
            np.testing.assert_allclose(_objective(z[f"{kind}_field_r"], st, d, s), j, rtol=1e-13)
