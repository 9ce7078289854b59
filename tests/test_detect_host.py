"""CPU checks of source detection: the numpy restatement of DESIGN 7e (tests/detect_oracle.py) on synthetic fields and
the DC2 fields of tests/golden/detect.npz, and the host side of detect_objects, Context.scene_detect and
IterativeDeblendField."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import detect_oracle as do

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _gauss(shape, cy, cx, sig, amp):
    y, x = np.mgrid[:shape[0], :shape[1]]
    return amp * np.exp(-0.5 * ((x - cx) ** 2 + (y - cy) ** 2) / sig ** 2)


def _golden():
    return np.load(os.path.join(HERE, "golden", "detect.npz"))


def test_background_recovers_level_and_rms_with_partial_meshes():
    rng = np.random.default_rng(0)
    data = 10.0 + rng.normal(0, 2.0, size=(200, 259))       # 200 = 3 * 64 + 8 rows, 259 = 4 * 64 + 3 columns
    bk = do.background(data)
    assert bk["mesh_back"].shape == (4, 5)
    assert np.abs(bk["back"] - 10.0).max() < 0.2
    assert abs(bk["globalrms"] - 2.0) < 0.06
    assert np.abs(bk["rms"] - 2.0).max() < 0.2
    small = do.background(data[:20, :30])                    # a field smaller than one mesh: one constant mesh
    assert small["mesh_back"].shape == (1, 1) and np.ptp(small["back"]) == 0.0


def test_mesh_statistics_clip_an_outlier():
    v = np.concatenate([np.linspace(-1.0, 1.0, 101), [1.0e3]])
    back, rms = do.mesh_stats(v)
    assert abs(back) < 1e-12 and abs(rms - np.std(np.linspace(-1.0, 1.0, 101))) < 1e-12


def test_spline_interpolates_and_extends_its_end_cubics():
    y = np.array([1.0, 3.0, 2.0, 5.0])
    m = do.spline_d2(y)
    assert m[0] == 0.0 and m[-1] == 0.0
    np.testing.assert_allclose(do.spline_eval(y, m, np.arange(4.0)), y, rtol=0, atol=1e-14)
    np.testing.assert_array_equal(do.spline_eval(np.array([2.0]), np.zeros(1), np.array([-3.0, 5.0])), [2.0, 2.0])
    np.testing.assert_allclose(do.spline_eval(np.array([0.0, 1.0]), np.zeros(2), np.array([-1.0, 2.5])), [-1.0, 2.5])


def test_default_kernel_matches_the_reference_table():
    """the pixel-integrated Gaussian (sigma 1.27627) scaled to the table's centre tap: within 2e-6 of every tap (9e-7
    measured)"""
    t = _golden()["ref_filter"]
    k = do.default_kernel()
    assert k.shape == t.shape == (7, 7)
    assert np.abs(k * (t[3, 3] / k[3, 3]) - t).max() < 2e-6


def test_two_gaussians_seven_pixels_apart_are_deblended():
    rng = np.random.default_rng(1)
    f = rng.normal(0, 1, (128, 128)) + _gauss((128, 128), 60, 60, 2.0, 40.0) + _gauss((128, 128), 60, 67, 2.0, 40.0)
    c = do.detect(f)
    assert len(c["x"]) == 2 and c["parent"][0] == c["parent"][1]
    np.testing.assert_allclose(c["x"], [60.0, 67.0], atol=0.2)
    np.testing.assert_allclose(c["y"], [60.0, 60.0], atol=0.2)
    one = do.detect(f, cont=1.0)
    assert len(one["x"]) == 1 and one["npix"][0] == c["npix"].sum()


def test_pure_noise_gives_no_detection():
    rng = np.random.default_rng(2)
    assert len(do.detect(rng.normal(0, 1, (256, 256)))["x"]) == 0      # measured: 0


@pytest.mark.parametrize("k,found,total,objects", [(2, 37, 40, 56), (3, 23, 27, 37)])
def test_oracle_recall_on_dc2_fields(k, found, total, objects):
    """truth galaxies with a detection within 2 px (crude smoothed-peak baseline: 37/40 and 23/27); counts pinned as
    measured"""
    z = _golden()
    f = z[f"field{k}_r"].astype(np.float64)
    tr, (cx, cy) = z[f"truth{k}"], z[f"center{k}"]
    F = f.shape[0]
    c = do.detect(f)
    rows, cols = tr[:, 1] - cy + F // 2, tr[:, 0] - cx + F // 2
    d = np.hypot(rows[:, None] - c["y"][None], cols[:, None] - c["x"][None]).min(axis=1)
    assert len(tr) == total and int((d <= 2.0).sum()) == found and len(c["x"]) == objects


def test_detect_objects_rounds_half_to_even_and_centres():
    from debvader_amd.detect.detection import _distances

    F = 259
    out = _distances(np.array([129.5, 130.5, 0.0]), np.array([128.5, 129.49, 258.0]), F)
    np.testing.assert_array_equal(out, [[0.0, 0.0], [0.0, 2.0], [129.0, -129.0]])
    assert _distances(np.array([]), np.array([]), F).shape == (0,)
    # the oracle's restatement of the reference's function rounds the same way
    z = _golden()
    img = np.zeros((1, 259, 259, 3))
    img[0, :, :, 2] = z["field2_r"]
    ref = do.detect_objects(img)
    c = do.detect(img[0, :, :, 2])
    np.testing.assert_array_equal(ref, _distances(c["x"], c["y"], 259))


def test_argument_checks_fail_before_the_gpu():
    from debvader_amd import engine as E
    from debvader_amd.detect.detection import detect_objects, detect_objects_batch

    f = np.zeros((1, 32, 32))
    base = dict(thresh=1.5, minarea=4, nthresh=64, cont=1e-5, filter_kernel=None, back_size=64, back_filter=3)
    for bad in (dict(minarea=0), dict(nthresh=0), dict(back_size=65), dict(back_filter=2),
                dict(filter_kernel=np.ones((4, 3))), dict(filter_kernel=np.ones((17, 17))),
                dict(filter_kernel=np.zeros((3, 3))), dict(thresh=np.nan)):
        with pytest.raises(ValueError):
            E.check_detect_args(f, **{**base, **bad})
    with pytest.raises(ValueError, match="finite"):
        E.check_detect_args(np.full((1, 8, 8), np.nan), **base)
    with pytest.raises(ValueError, match=r"\(M, H, W\)"):
        E.check_detect_args(np.zeros((8, 8)), **base)
    with pytest.raises(ValueError, match="band"):
        detect_objects(np.zeros((1, 32, 32, 2)))
    with pytest.raises(ValueError, match="band"):
        detect_objects_batch(np.zeros((2, 32, 32, 1)))


def test_entry_point_and_reference_signatures():
    from debvader_amd import _lib
    from debvader_amd.deblend.field_deblender import DeblendField
    from debvader_amd.deblend_iterative.iterative_deblender import IterativeDeblendField
    from debvader_amd.detect import detection

    assert "dv_scene_detect" in _lib.SIGNATURES and hasattr(_lib.lib, "dv_scene_detect")
    assert list(inspect.signature(detection.detect_objects).parameters)[0] == "field_image"
    assert issubclass(IterativeDeblendField, DeblendField)
    assert list(inspect.signature(IterativeDeblendField.iterative_deblending).parameters) == [
        "self", "galaxy_distances_to_center", "cutout_images", "optimise_positions", "epistemic_criterion",
        "mse_criterion"]
    assert list(inspect.signature(IterativeDeblendField.deblending_step).parameters) == [
        "self", "field_image", "cutout_images", "optimise_positions", "epistemic_criterion", "mse_criterion"]


def test_root_name_points_to_the_iterative_deblender():
    code = ("import debvader_amd\n"
            "try:\n    debvader_amd.IterativeDeblendField\n    raise SystemExit('no error')\n"
            "except NotImplementedError as e:\n"
            "    m = str(e)\n"
            "    assert 'sep' in m and 'SExtractor' in m, m\n"
            "    assert 'debvader_amd.deblend_iterative.iterative_deblender.IterativeDeblendField' in m, m\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
