"""CPU tests of which combinations of the catalogue extras DeblendFieldBatch.deblend_fields refuses - the Monte-Carlo errors,
blendedness, PSF-corrected shapes, aperture photometry and the flux fit - over the stand-in engine of
tests/stub_fit_flux_engine.py.  No GPU, no HIP.  The extras are listed here by hand, not read from the product's table: the
set of refusals is what the table has to reproduce."""
import itertools

import numpy as np
import pytest

from tests.stub_fit_flux_engine import CS, NB, Net

F = 81
DIST = [np.array([[0.0, 0.0], [5.0, -7.0]]), np.zeros((0, 2)), np.array([[-3.0, 11.0]])]
EXTRAS = [dict(measure_samples=4), dict(blendedness=True), dict(psf=np.ones((21, 21))), dict(apertures=(3.0,)),
          dict(fit_flux=True)]
ON = dict(on_device=True, measure=True)


def _batch():
    from debvader_amd.deblend.field_deblender import DeblendFieldBatch

    net = Net()
    return net, DeblendFieldBatch(net, np.random.default_rng(3).normal(size=(3, F, F, NB)), CS, NB)


def _engine_calls(net):
    return [c for c in net._core.engine.calls if c[0].startswith("infer")]


def test_any_two_extras_are_refused_together():
    net, b = _batch()
    pairs = list(itertools.combinations(EXTRAS, 2))
    assert len(pairs) == 10
    for first, second in pairs:
        for kw in ({**first, **second}, {**second, **first}):
            with pytest.raises(ValueError, match="cannot be combined with"):
                b.deblend_fields(DIST, **ON, **kw)
            with pytest.raises(ValueError, match="cannot be combined with"):
                b.deblend_fields(DIST, **ON, return_fields=False, **kw)
    assert _engine_calls(net) == [] and net._core.seed_counter == 7


def test_every_extra_is_refused_in_the_passes_without_a_catalogue_stage():
    net, b = _batch()
    for extra in EXTRAS:
        (name,) = extra
        for other in ("optimise_positions", "epistemic_uncertainty_estimation"):
            with pytest.raises(ValueError, match=f"{name}.* cannot be combined with .*{other}"):
                b.deblend_fields(DIST, **ON, **extra, **{other: True})
    assert _engine_calls(net) == [] and net._core.seed_counter == 7


def test_every_extra_needs_the_measuring_on_device_call():
    net, b = _batch()
    for extra in EXTRAS:
        (name,) = extra
        for kw in (dict(), dict(measure=True), dict(on_device=True)):
            with pytest.raises(ValueError, match=f"{name}.* needs? (measure|on_device)=True"):
                b.deblend_fields(DIST, **kw, **extra)
    assert _engine_calls(net) == [] and net._core.seed_counter == 7


def test_apertures_with_aperture_data_is_the_one_pair_that_passes():
    net, b = _batch()
    # the stand-in engine has no aperture call: getting as far as asking it for one is getting past the refusals
    with pytest.raises(AttributeError, match="infer_fields_measure_aper_data"):
        b.deblend_fields(DIST, **ON, apertures=(3.0,), aperture_data=True)
    with pytest.raises(AttributeError, match="infer_fields_measure_aper'"):
        b.deblend_fields(DIST, **ON, apertures=(3.0,))
    # aperture_data is no extra of its own: without apertures it is refused, and beside them it changes no other refusal
    with pytest.raises(ValueError, match="aperture_data=True needs apertures"):
        b.deblend_fields(DIST, **ON, aperture_data=True)
    for extra in EXTRAS:
        if "apertures" not in extra:
            with pytest.raises(ValueError, match="cannot be combined with"):
                b.deblend_fields(DIST, **ON, apertures=(3.0,), aperture_data=True, **extra)
    assert _engine_calls(net) == []
