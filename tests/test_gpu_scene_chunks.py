"""The chunk walkers of the stand-alone catalogue calls (csrc/rows.hip): a call cut into chunks of stamps and groups of
fields - or, for the flux fits and the moments on the fields, into runs of whole fields - gives the bits of the call that goes
through in one piece.

Free device memory holds any test input many times over, so the second chunk of these loops - the list cut at a chunk or
field-group boundary, every host row offset by the chunk's base - is reached only under dv_debug_scene_limits of the
development build (tests/debug_lib.py).  The uncapped run is the reference; what the values should be is the business of the
test files of each call.

The smallest input that crosses every kind of boundary: 5 stamps of 9 x 9 pixels and 2 bands in 3 fields of 16 pixels with
field_ptr (0, 2, 2, 5) - the middle field is empty and a cap of 2 cuts inside the last -, one ineligible catalogue row (an
all-zero stamp), one stamp partly outside its field, 2 PSFs of 7 pixels, 3 Monte-Carlo samples, one stack of weight fields
(positive, a few zeros, one inf).  The calls that take whole fields at a time are cut by the same caps into one field per run
- field 2 goes through with its three rows on the at-least-one-field rule, and a sky fit visits the run of the empty field 1 -
and into fields 0 - 1, then field 2.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import debug_lib

pytestmark = pytest.mark.gpu

N, CS, NB, M, F, S, BAND = 5, 9, 2, 3, 16, 3, 1
FIELD_PTR = np.array([0, 2, 2, 5], np.int64)
CAPS = ((2, 1), (3, 2))               # (stamps, fields): chunks of 2 + 2 + 1 in one field each; 2 + 3, the first of two fields
#                                       (whole fields at a time: fields 0 | 1 | 2; fields 0 - 1 | 2)
RADII, FRACTIONS, SUBSAMPLE = (1.5, 2.5), (0.5,), 3


def _blob(cs, r0, c0, s_r, s_c, amp):
    r, c = np.mgrid[0:cs, 0:cs].astype(np.float64)
    return amp * np.exp(-0.5 * (((r - r0) / s_r) ** 2 + ((c - c0) / s_c) ** 2))


@functools.lru_cache(maxsize=None)
def _inputs():
    """(mean, stddev float32 (N, CS, CS, NB), samples float32 (S, N, CS, CS, NB), places, psf, psf_index, model, data, weights)"""
    rng = np.random.default_rng(77)
    mean = np.zeros((N, CS, CS, NB), np.float32)
    blobs = [(4.0, 4.0, 1.4, 1.4), (3.6, 4.3, 1.2, 1.7), None, (4.4, 3.8, 1.6, 1.3), (4.1, 4.2, 1.3, 1.3)]
    for i, b in enumerate(blobs):                     # stamp 2 stays all zero: no positive weighted flux, status 3
        if b is not None:
            for band in range(NB):
                mean[i, :, :, band] = _blob(CS, *b, amp=10.0 * (band + 1) + i)
    stddev = (0.05 + 0.01 * rng.random(mean.shape)).astype(np.float32)
    samples = (mean[None] + 0.02 * rng.standard_normal((S,) + mean.shape)).astype(np.float32)
    samples[:, 2] = 0.0
    places = np.array([[2, 3], [6, 1], [4, 4], [-3, 10], [5, 5]], np.int32)     # stamp 3 hangs over the top and the right edge
    psf = np.stack([_blob(7, 3.0, 3.0, 0.9, 0.9, 1.0), _blob(7, 3.0, 3.0, 1.0, 0.8, 1.0) + 0.01 * _blob(7, 2.0, 4.0, 0.6, 0.6, 1.0)])
    psf /= psf.sum(axis=(1, 2), keepdims=True)
    psf_index = np.array([0, 1, 0, 1, 1], np.int32)
    model = rng.random((M, F, F, NB))
    data = model + 0.1 * rng.standard_normal(model.shape)
    weights = rng.uniform(0.25, 4.0, size=model.shape)           # (drawn last: the inputs above keep their values)
    weights[rng.random(model.shape) < 0.05] = 0.0
    weights[2, 7, 12, 1] = np.inf                                # field 2, under stamps 2 and 4
    for a in (mean, stddev, samples, places, psf, psf_index, model, data, weights):
        a.setflags(write=False)
    return mean, stddev, samples, places, psf, psf_index, model, data, weights


def _calls(ctx):
    """name -> the call, every input fixed; the catalogue and aperture rows the later calls read are measured here, uncapped"""
    mean, stddev, samples, places, psf, psf_index, model, data, weights = _inputs()
    cat = ctx.scene_measure(mean, band=BAND)
    assert cat["status"][2] == 3 and set(np.delete(cat["status"], 2)) <= {0, 2}      # one ineligible row among eligible ones
    shape, status = cat["shape"], cat["status"]
    ap = ctx.scene_aperture(mean, shape, status, radii=RADII, fractions=FRACTIONS, band=BAND, subsample=SUBSAMPLE)
    akw = dict(radii=RADII, fractions=FRACTIONS, band=BAND, subsample=SUBSAMPLE)
    fkw = dict(field_ptr=FIELD_PTR, cutout_size=CS, radii=RADII, subsample=SUBSAMPLE)
    fit = (mean, places, data)
    wkw = dict(field_ptr=FIELD_PTR, weight_fields=weights)
    return {
        "measure": lambda: ctx.scene_measure(mean, band=BAND),
        "measure_stddev": lambda: ctx.scene_measure(mean, stddev, band=BAND),
        "measure_mc": lambda: ctx.scene_measure_mc(samples, band=BAND),
        "measure_mc_keep": lambda: ctx.scene_measure_mc(samples, band=BAND, keep_samples=True),
        "regauss": lambda: ctx.scene_regauss(mean, shape, status, psf, psf_index, band=BAND),
        "aperture": lambda: ctx.scene_aperture(mean, shape, status, **akw),
        "aperture_stddev": lambda: ctx.scene_aperture(mean, shape, status, stddev, **akw),
        "blend": lambda: ctx.scene_blend(mean, shape, status, places, model, field_ptr=FIELD_PTR, band=BAND),
        "blend_data": lambda: ctx.scene_blend(mean, shape, status, places, model, data, field_ptr=FIELD_PTR, band=BAND),
        "aperture_fields": lambda: ctx.scene_aperture_fields(shape, status, places, ap["kron"], ap["aper_status"], model, **fkw),
        "aperture_fields_data": lambda: ctx.scene_aperture_fields(shape, status, places, ap["kron"], ap["aper_status"], model,
                                                                  data, **fkw),
        "fit_flux": lambda: ctx.scene_fit_flux(*fit, field_ptr=FIELD_PTR),
        "fit_flux_weighted": lambda: ctx.scene_fit_flux(*fit, **wkw),
        "fit_flux_sky0": lambda: ctx.scene_fit_flux_sky(*fit, field_ptr=FIELD_PTR, sky_order=0),
        "fit_flux_sky1_weighted": lambda: ctx.scene_fit_flux_sky(*fit, sky_order=1, **wkw),
        "fit_flux_nonneg_sky1_weighted": lambda: ctx.scene_fit_flux_nonneg(*fit, sky_order=1, **wkw),
        "fit_flux_nonneg": lambda: ctx.scene_fit_flux_nonneg(*fit, field_ptr=FIELD_PTR),
        "fit_flux_groups": lambda: ctx.scene_fit_flux_groups(*fit, field_ptr=FIELD_PTR),
        "fit_flux_groups_weighted": lambda: ctx.scene_fit_flux_groups(*fit, **wkw),
        "moments_fields_weighted": lambda: ctx.scene_moments_fields(mean, places, model, data, weights, field_ptr=FIELD_PTR, band=BAND),
        "moments_fields": lambda: ctx.scene_moments_fields(mean, places, model, data, field_ptr=FIELD_PTR, band=BAND),
    }


CALLS = ("measure", "measure_stddev", "measure_mc", "measure_mc_keep", "regauss", "aperture", "aperture_stddev", "blend",
         "blend_data", "aperture_fields", "aperture_fields_data", "fit_flux", "fit_flux_weighted", "fit_flux_sky0",
         "fit_flux_sky1_weighted", "fit_flux_nonneg_sky1_weighted", "fit_flux_nonneg", "fit_flux_groups",
         "fit_flux_groups_weighted", "moments_fields_weighted", "moments_fields")


@pytest.mark.parametrize("name", CALLS)
def test_a_call_cut_into_chunks_gives_the_bits_of_the_whole_call(name):
    from debvader_amd import engine as E
    from debvader_amd._lib import check

    with debug_lib.debug_build() as dlib:
        call = _calls(E.default_context())[name]
        want = call()
        assert want and all(v.shape[0] in (N, M, 2) for v in want.values())         # (2: the PSFs' own rows; M: per field)
        for caps in CAPS:
            check(dlib.dv_debug_scene_limits(*caps))
            try:
                got = call()
            finally:
                check(dlib.dv_debug_scene_limits(0, 0))
            assert sorted(got) == sorted(want)
            for k in want:                                  # bit for bit, NaN positions (and payloads) included
                assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (name, caps, k)
    if name == "measure":
        assert np.isfinite(want["shape"][[0, 1, 3, 4]]).all()
    if name.startswith("blend"):                            # the inputs do what the docstring says they do
        assert want["npix"][2] == -1 and 0 < want["npix"][3] < CS * CS and np.isnan(want["blend"][2]).all()


def test_a_capped_call_refuses_what_the_uncapped_call_refuses():
    """the field_ptr cases of tests/test_gpu_blend.py and tests/test_gpu_aperture_fields.py: the same message, capped or not"""
    from debvader_amd import engine as E
    from debvader_amd._lib import DvError, check
    from debvader_amd.engine import _dp, _fp, _ip, aperture_params

    i64 = lambda a: np.asarray(a, np.int64).ctypes.data_as(C.POINTER(C.c_int64))     # noqa: E731
    st = np.zeros((3, CS, CS, 3), np.float32)
    sh, ss, kr, pl = np.zeros((3, 5)), np.zeros(3, np.int32), np.zeros((3, 3)), np.zeros((3, 2), np.int32)
    T, bl, npx = np.zeros((2, 40, 40, 3)), np.zeros((3, 4)), np.zeros(3, np.int32)
    six = [np.zeros((3, 3, 3)), np.zeros((3, 3, 3)), np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3)]
    apar = aperture_params()
    far = np.array([[0, 0], [1 << 29, 0], [0, 0]], np.int32)

    with debug_lib.debug_build() as dlib:
        ctx = E.default_context()

        def blend(fptr, n=3, places=pl):
            check(dlib.dv_scene_blend(ctx._h, _fp(st), _dp(sh), _ip(ss), _ip(places), i64(fptr), n, CS, 3, 2, _dp(T), None, 2, 40,
                                      _dp(bl), _ip(npx)))

        def fields(fptr, n=3, places=pl):
            check(dlib.dv_scene_aperture_fields(ctx._h, _dp(sh), _ip(ss), _ip(places), i64(fptr), _dp(kr), _ip(ss), n, 31, 3,
                                                _dp(T), _dp(T), 2, 40, C.byref(apar), *map(_dp, six)))

        def message(call, *a, **kw):
            with pytest.raises(DvError) as e:
                call(*a, **kw)
            return str(e.value)

        cases = [(blend, dict(fptr=(0, 1, 2)), "field_ptr must run from 0"), (blend, dict(fptr=(0, 1 << 40, 3)), "decreases at field 1"),
                 (blend, dict(fptr=(0, 2, 3), places=far), "placement 1"),
                 (fields, dict(fptr=(1, 2, 3)), "field_ptr must run from 0"), (fields, dict(fptr=(0, 2, 4)), "field_ptr must run from 0"),
                 (fields, dict(fptr=(0, 4, 3)), "decreases at field 1"), (fields, dict(fptr=(0, -1, 3)), "decreases at field 0"),
                 (fields, dict(fptr=(0, 2, 3), places=far), "placement 1")]
        want = [message(call, **kw) for call, kw, _ in cases]
        for (_, _, part), w in zip(cases, want):
            assert part in w, w
        check(dlib.dv_debug_scene_limits(2, 1))
        try:
            got = [message(call, **kw) for call, kw, _ in cases]
            blend((0, 2, 3))                                 # and a correct call goes through, in two chunks
            fields((0, 2, 3))
        finally:
            check(dlib.dv_debug_scene_limits(0, 0))
        assert got == want
