"""Field deblending around the network (reference: src/debvader/deblend/field_deblender.py).

Same class and method names as the reference.  What runs on the GPU: cutout extraction, the network
(`deblend`), the epistemic Monte-Carlo estimate (one engine call for all objects instead of a Python loop of
100-stamp batches) and the residual / predicted field compositing (instead of one scipy.ndimage.shift of a
field-sized image per object and band) and the sub-pixel position fit (deblend_cutout/optimization.py, one batched engine
call for all galaxies instead of a scipy.optimize run per galaxy): `optimise_positions()` fits the rows of a deblended
recarray and writes their `shifts`.  `deblend_field(optimise_positions=True)` still raises: run `deblend_field` and then
`optimise_positions()`.  Source detection: debvader_amd.detect.detection (SExtractor's method on the GPU, not sep).
"""
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional

import numpy as np
import pandas as pd

from debvader_amd import engine as E
from debvader_amd.deblend_cutout.deblender import deblend, deblend_epistemic
from debvader_amd.extract.extraction import cutout_windows, extract_cutouts  # noqa: F401  (extract_cutouts: re-exported as in the reference)
from debvader_amd.measure import measurement as ms
from debvader_amd.training.metrics import mse  # noqa: F401  (the reference's module imports it; the cut below is its vector form)


def _to_records(cols):
    """`pd.DataFrame(cols).to_records(index=False)` (field_deblender.py:380) without pandas walking the per-galaxy image
    columns: the scalar columns go through pandas (its dtype inference: int64 / float64 / bool), the columns whose entries
    are arrays become object columns directly.  Same recarray - dtype, field order, entries (tests/test_scene.py) - in a
    tenth of the time at 32 768 galaxies per call."""
    names = list(cols)
    n = len(cols[names[0]])
    obj = [k for k in names if n and isinstance(cols[k][0], np.ndarray)]
    rest = pd.DataFrame({k: cols[k] for k in names if k not in obj}).to_records(index=False)
    out = np.recarray((n,), dtype=[(k, "O") if k in obj else (k, rest.dtype[k]) for k in names])
    for k in names:
        if k in obj:
            col = np.empty(n, dtype=object)
            for i, a in enumerate(cols[k]):
                col[i] = a
            out[k] = col
        else:
            out[k] = rest[k]
    return out


class _Extra(NamedTuple):
    """One optional part of the on-device catalogue of DeblendFieldBatch.deblend_fields: a keyword, the engine call that
    serves it and what it appends to the recarrays.  `c` below is the namespace of one call: bands, band, sky_sigma,
    field_ptr, psf, psf_index, aper_par, nmc, fit_weights, fit_sky, moments_weights, places, cs, F, core."""
    key: str                        # the keyword of deblend_fields
    given: Callable                 # its value -> whether the extra is asked for
    label: str                      # how a message names it
    verb: str                       # ... "needs" / "need" measure=True and on_device=True
    what: str                       # what the engine call adds, as a message names it
    why: str                        # why it needs the measuring on-device call, and what to use on the default path
    call: str                       # the C call, named in messages
    method: str                     # the Engine method
    places_always: bool             # whether the catalogue-only form passes the placements too
    kwargs: Callable                # c -> the keyword arguments of the engine call beside places, seed and return_fields
    columns: Callable               # c -> what it appends to the recarrays' dtype
    records: Callable               # (out, c) -> the recarray of those columns, rows = global stamp numbers
    orphans: tuple = ()             # ((keyword, message), ...): keywords that are refused without this one
    refines: Optional[str] = None   # the key of the extra this one goes with and whose engine call it replaces; `why` is
                                    # then the refusal without it


def _fit_weight_records(out, c):
    """What fit_weights appends behind the columns of fit_flux: the last two columns of fit_flux_weighted_dtype"""
    rec = np.recarray((len(out["fit_chi2"]),), dtype=ms.fit_flux_weighted_dtype(c.bands)[len(ms.fit_flux_dtype(c.bands)):])
    rec["fit_chi2"], rec["fit_npix"] = out["fit_chi2"], out["fit_npix"]
    return rec


def _aper_kwargs(c):
    return dict(radii=list(c.aper_par.radii)[:c.aper_par.n_radii], fractions=list(c.aper_par.fractions)[:c.aper_par.n_fractions])


# In the order the extras were added, which is the order of their columns.  Any two are refused together (the later one
# speaks), but for an extra and the one that refines it.
_EXTRAS = (
    _Extra("measure_samples", lambda v: bool(int(v or 0)), "measure_samples", "needs", "the Monte-Carlo catalogue",
           "the Monte-Carlo decodes are measured where they lie in device memory",
           "dv_infer_fields_measure_mc", "infer_fields_measure_mc", False,
           lambda c: dict(mc_seed=c.core.next_seed(), nsamples=c.nmc),
           lambda c: ms.catalogue_mc_dtype(c.bands),
           lambda out, c: ms.catalogue_mc_records(out["flux_mc_mean"], out["flux_mc_std"], out["shape_mc_mean"],
                                                  out["shape_mc_std"], out["n_ok"])),
    _Extra("blendedness", bool, "blendedness=True", "needs", "the blendedness sums",
           "the weight of the sums is the Gaussian of the measured adaptive moments, and they are taken where the stamps and "
           "the composited fields lie in device memory (dv_infer_fields_measure_blend); on the default path use "
           "debvader_amd.measure.measurement.measure_blendedness on the returned stamps",
           "dv_infer_fields_measure_blend", "infer_fields_measure_blend", True,
           lambda c: {},
           lambda c: ms.blend_dtype(),
           lambda out, c: ms.blend_records(out["blend"], out["npix"])),
    _Extra("psf", lambda v: v is not None, "psf", "needs", "the PSF correction",
           "the correction starts from the measured adaptive moments and runs where the stamps lie in device memory "
           "(dv_infer_fields_measure_psf); on the default path use debvader_amd.measure.measurement.measure_stamps_psf on the "
           "returned stamps",
           "dv_infer_fields_measure_psf", "infer_fields_measure_psf", False,
           lambda c: dict(psf=c.psf, psf_index=c.psf_index),
           lambda c: ms.psf_dtype(),
           lambda out, c: ms.psf_records(out["regauss"], out["regauss_iters"], out["regauss_status"], out["psf_shape"],
                                         out["psf_aux"], c.psf_index),
           orphans=(("psf_index", "psf_index picks a galaxy's image out of psf: give psf too"),)),
    _Extra("apertures", lambda v: v is not None, "apertures", "need", "the aperture photometry",
           "the apertures are centred on the measured centroid and taken where the stamps lie in device memory "
           "(dv_infer_fields_measure_aper); on the default path use debvader_amd.measure.measurement.measure_apertures on the "
           "returned stamps",
           "dv_infer_fields_measure_aper", "infer_fields_measure_aper", False,
           _aper_kwargs,
           lambda c: ms.aperture_dtype(c.bands, c.aper_par.n_radii, c.aper_par.n_fractions),
           lambda out, c: ms.aperture_records(*(out[k] for k in E.APERTURE_KEYS), out["shape"]),
           orphans=(("flux_fractions", "flux_fractions are fractions of the Kron flux of the aperture photometry: give apertures "
                                       "too (apertures=() for the Kron columns alone)"),)),
    _Extra("aperture_data", bool, "aperture_data=True", "needs", "the apertures on the fields",
           "aperture_data=True needs apertures: it takes the apertures of the aperture photometry on the observed field and the "
           "composited mean field (apertures=() for the Kron ellipse alone)",
           "dv_infer_fields_measure_aper_data", "infer_fields_measure_aper_data", True,
           lambda c: dict(band=c.band, **_aper_kwargs(c)),
           lambda c: ms.aperture_data_dtype(c.bands, c.aper_par.n_radii),
           lambda out, c: ms.aperture_data_records(*(out[k] for k in E.APERTURE_FIELD_KEYS), out["ap_flux"], out["ap_area"],
                                                   out["flux_auto"], out["kron"][:, 2], band=c.band, sky_sigma=c.sky_sigma,
                                                   field_ptr=c.field_ptr),
           refines="apertures"),
    _Extra("fit_flux", bool, "fit_flux=True", "needs", "the flux fit",
           "the fit scales the measured stamp fluxes and runs where the mean stamps and the observed fields lie in device "
           "memory (dv_infer_fields_measure_fit); on the default path use debvader_amd.measure.measurement.fit_fluxes on the "
           "returned stamps",
           "dv_infer_fields_measure_fit", "infer_fields_measure_fit", True,
           lambda c: dict(band=c.band),
           lambda c: ms.fit_flux_dtype(c.bands),
           lambda out, c: ms.fit_flux_records(*(out[k] for k in E.FIT_FLUX_KEYS), out["flux"], sky_sigma=c.sky_sigma,
                                              field_ptr=c.field_ptr, weighted=c.fit_weights is not None)),
    _Extra("fit_weights", lambda v: v is not None, "fit_weights", "need", "the weighted flux fit",
           "fit_weights needs fit_flux=True: they are the per-pixel inverse variances (0 where a pixel is masked) the flux fit "
           "weights the observed pixels with",
           "dv_infer_fields_measure_fit_weighted", "infer_fields_measure_fit_weighted", True,
           lambda c: dict(band=c.band, weight_fields=c.fit_weights),
           lambda c: ms.fit_flux_weighted_dtype(c.bands)[len(ms.fit_flux_dtype(c.bands)):],
           lambda out, c: _fit_weight_records(out, c),
           refines="fit_flux"),
    # (behind fit_weights, whose call it replaces: it passes the weights on.  deblend_fields refuses it together with the two
    # refining extras below, so its call is never replaced by theirs)
    _Extra("fit_groups", bool, "fit_groups=True", "needs", "the flux fit by blend groups",
           "fit_groups=True needs fit_flux=True: it solves the flux fit blend group by blend group, without a limit on the "
           "galaxies of a field",
           "dv_infer_fields_measure_fit_groups", "infer_fields_measure_fit_groups", True,
           lambda c: dict(band=c.band, weight_fields=c.fit_weights),
           lambda c: ms.fit_groups_dtype(c.bands),
           lambda out, c: ms.fit_groups_records(out["fit_group"], out["fit_group_size"]),
           refines="fit_flux"),
    # (behind fit_weights, which refines the same extra: the call of the LAST refining extra given serves the others too - this
    # one passes the weights on)
    _Extra("fit_sky", lambda v: v is not None, "fit_sky", "needs", "the flux fit with a sky background",
           "fit_sky needs fit_flux=True: it is the order (0: a constant, 1: a plane) of the sky background the flux fit fits "
           "jointly with the amplitudes",
           "dv_infer_fields_measure_fit_sky", "infer_fields_measure_fit_sky", True,
           lambda c: dict(band=c.band, sky_order=c.fit_sky, weight_fields=c.fit_weights),
           lambda c: ms.fit_sky_dtype(c.bands),
           lambda out, c: ms.fit_sky_records(out["sky_coef"], out["sky_cov"], out["sky_status"], c.places, c.cs, c.F,
                                             field_ptr=c.field_ptr, sky_sigma=c.sky_sigma, weighted=c.fit_weights is not None),
           refines="fit_flux"),
    # (behind every extra that stands alone, so it speaks in every refusal beside one of them; it is combined with none, so its
    # columns meet no others.  fit_nonneg stays the last row: it refines, and its call replaces those of the rows before it)
    _Extra("moments_data", bool, "moments_data=True", "needs", "the moments on the observed field",
           "the adaptive moments are re-measured on the observed field with the neighbours' models subtracted where the mean "
           "stamps, the composited field and the observed field lie in device memory "
           "(dv_infer_fields_measure_moments_data); on the default path use "
           "debvader_amd.measure.measurement.measure_moments_on_fields on the returned stamps",
           "dv_infer_fields_measure_moments_data", "infer_fields_measure_moments_data", True,
           lambda c: dict(band=c.band, weight_fields=c.moments_weights),
           lambda c: ms.moments_data_dtype(c.bands),
           lambda out, c: ms.moments_data_records(out["flux_data"], out["npix_data"], out["shape_data"], out["iters_data"],
                                                  out["status_data"], sky_sigma=c.sky_sigma, field_ptr=c.field_ptr),
           orphans=(("moments_weights", "moments_weights are the mask of the moments on the observed field: give "
                                        "moments_data=True too"),)),
    # (the last refining extra: its call passes the weights and the order of the sky on - None: no sky)
    _Extra("fit_nonneg", bool, "fit_nonneg=True", "needs", "the non-negative flux fit",
           "fit_nonneg=True needs fit_flux=True: it constrains the amplitudes of the flux fit to be >= 0",
           "dv_infer_fields_measure_fit_nonneg", "infer_fields_measure_fit_nonneg", True,
           lambda c: dict(band=c.band, sky_order=c.fit_sky, weight_fields=c.fit_weights),
           lambda c: ms.fit_nonneg_dtype(c.bands),
           lambda out, c: ms.fit_nonneg_records(*(out[k] for k in E.FIT_NONNEG_KEYS), out["flux"]),
           refines="fit_flux"),
)


def _refuse_extra(x, kw, given, measure, on_device, fit, mc):
    """The refusals of extra `x` of a deblend_fields call with keywords `kw`: what is given without it, the call it needs,
    every older extra beside it, and the passes that have no catalogue stage.  given: the keys of the extras asked for."""
    for key, message in x.orphans:
        if kw[key] is not None and x.key not in given:
            raise ValueError(message)
    if x.key not in given:
        return
    if x.refines:
        if x.refines not in given:
            raise ValueError(x.why)
        return
    if not (measure and on_device):
        lacks = " and ".join(k for k, v in (("measure=True", measure), ("on_device=True", on_device)) if not v)
        raise ValueError(f"{x.label} {x.verb} measure=True and on_device=True: {x.why}.  Here {x.label} {x.verb} {lacks}")
    for y in reversed(_EXTRAS[:_EXTRAS.index(x)]):
        if y.key in given and not y.refines:
            raise ValueError(f"{x.label} cannot be combined with {y.label}: {x.what} and {y.what} are stages of two different "
                             f"measuring calls ({x.call}, {y.call})")
    for on, other, kind in ((fit, "optimise_positions=True", "position-fit"), (mc, "epistemic_uncertainty_estimation=True",
                                                                              "Monte-Carlo")):
        if on:
            raise ValueError(f"{x.label} cannot be combined with {other}: only the plain measuring composite call ({x.call}) "
                             f"has a stage for {x.what}, the {kind} call has none")


class DeblendField:
    def __init__(self, net, field_image, cutout_size=59, nb_of_bands=6, epistemic_uncertainty_estimation=False,
                 normalise=False):
        """
        parameters (field_deblender.py:14-44):
            net: network used to deblend the field
            field_image: image of the field to deblend, shape (1, size, size, bands)
            cutout_size: size of the stamps
            nb_of_bands: number of filters in the image
            epistemic_uncertainty_estimation: estimate the epistemic uncertainty with 100 stochastic passes per object
            normalise: normalise the stamps before the network
        """
        self.net = net
        self.field_image = np.array(field_image, dtype=np.float64, copy=True)
        self.field_size = field_image.shape[1]
        self.cutout_size = cutout_size
        self.nb_of_bands = nb_of_bands
        self.epistemic_uncertainty_estimation = epistemic_uncertainty_estimation
        self.normalise = normalise
        self.nb_of_detected_objects = []
        self.nb_of_deblended_galaxies = []
        self.res_deblend = None
        self.mse = []
        self._ctx_obj = getattr(getattr(net, "_core", None), "ctx", None)   # the compositing runs on the net's GPU context;
                                                                            # a net without one gets the default context at
                                                                            # the first get_*_field call (see _ctx)
        self._device_fields = None      # (recarray, fields composited on the GPU) of the last deblend_field(on_device=True)

    @property
    def _ctx(self):
        if self._ctx_obj is None:
            self._ctx_obj = E.default_context()
        return self._ctx_obj

    # -- compositing -------------------------------------------------------------------------------
    @staticmethod
    def _positions(res_deblend):
        return np.array([[row["galaxy_distances_to_center_x"] + row["shifts"][0],
                          row["galaxy_distances_to_center_y"] + row["shifts"][1]] for row in res_deblend],
                        dtype=np.float64).reshape(-1, 2)

    def _own_device_fields(self, res_deblend):
        """The fields an on-device pass composited, if `res_deblend` (None: self.res_deblend) is that pass's recarray."""
        if self._device_fields is None:
            return None
        rec, fields = self._device_fields
        if rec is self.res_deblend and (res_deblend is None or res_deblend is rec):
            return fields
        return None

    def _stack(self, res_deblend, key):
        names = getattr(getattr(res_deblend, "dtype", None), "names", None)
        if names is not None and key not in names:
            raise ValueError(f"this recarray has no {key!r} column: it comes from deblend_field(on_device=True), whose stamps "
                             "stayed on the GPU - only the object that made it can return its fields, and only until its next "
                             "pass; run the default path to composite from stamps")
        return np.array([np.asarray(row[key], dtype=np.float64) for row in res_deblend], dtype=np.float64).reshape(
            -1, self.cutout_size, self.cutout_size, self.nb_of_bands)

    def get_residual_field(self, res_deblend=None):
        """Field minus every predicted galaxy at its position (field_deblender.py:46-97); shape of the input field."""
        dev = self._own_device_fields(res_deblend)
        if dev is not None:
            return dev["residual_field"][None].copy()
        if res_deblend is None:
            res_deblend = self.res_deblend
        deblended_image = self.field_image.copy()
        if res_deblend is not None and len(res_deblend) > 0:
            deblended_image[0] = self._ctx.scene_composite(
                self.field_image[0], self._stack(res_deblend, "output_images_mean"), self._positions(res_deblend), -1.0)
        return deblended_image

    def get_predicted_field(self, res_deblend=None):
        """Predicted mean / stddev / epistemic fields (field_deblender.py:99-189), each (size, size, bands)."""
        dev = self._own_device_fields(res_deblend)
        if dev is not None:
            # deblend_field(on_device=True) composited them on the GPU behind the forward passes
            return {"predicted_mean_field": dev["mean_field"].copy(), "predicted_stddev_field": dev["stddev_field"].copy(),
                    "predicted_epistemic_field": dev["epistemic_field"].copy() if "epistemic_field" in dev
                    else np.zeros_like(dev["mean_field"])}
        if res_deblend is None:
            res_deblend = self.res_deblend
        zeros = np.zeros((self.field_size, self.field_size, self.nb_of_bands))
        out = {"predicted_mean_field": zeros.copy(), "predicted_stddev_field": zeros.copy(),
               "predicted_epistemic_field": zeros.copy()}
        if res_deblend is not None and len(res_deblend) > 0:
            pos = self._positions(res_deblend)
            out["predicted_mean_field"] = self._ctx.scene_composite(zeros, self._stack(res_deblend, "output_images_mean"), pos)
            out["predicted_stddev_field"] = self._ctx.scene_composite(zeros, self._stack(res_deblend, "output_images_stddev"), pos)
            if self.epistemic_uncertainty_estimation:
                out["predicted_epistemic_field"] = self._ctx.scene_composite(
                    zeros, self._stack(res_deblend, "epistemic_uncertainty"), pos)
        return out

    def get_deblending_meta_data(self, res_deblend=None):
        """field_deblender.py:191-217: the field, the residual and the three predicted fields in one dictionary."""
        meta = {"field_image": self.field_image, "deblended_image": self.get_residual_field(res_deblend)}
        meta.update(self.get_predicted_field(res_deblend))
        return meta

    # -- position fit ------------------------------------------------------------------------------
    def optimise_positions(self, res_deblend=None, field_image=None):
        """Fit the sub-pixel shift of every row of `res_deblend` (None: self.res_deblend) and write it to the `shifts` column.

        The reference's per-galaxy position_optimization (field_deblender.py:337-352, deblend_cutout/optimization.py) for
        all rows at once, whatever `passed_cuts` says, as the reference does: the r band of `field_image` (None:
        self.field_image) against each row's `output_images_mean` placed at its distance to the centre, shifts in
        [-3, 3]^2.  Each `shifts` entry becomes a float64 np.array([shift_x, shift_y]); get_residual_field() and
        get_predicted_field() then place the galaxies at distance + shift.  Returns the recarray.  A recarray from
        deblend_field(on_device=True) carries no stamps and raises ValueError."""
        from debvader_amd.deblend_cutout.optimization import position_optimization_batch

        if res_deblend is None:
            res_deblend = self.res_deblend
        if res_deblend is None or getattr(getattr(res_deblend, "dtype", None), "names", None) is None:
            raise ValueError("optimise_positions() needs the recarray of a deblend_field() pass")
        if len(res_deblend) == 0:
            return res_deblend
        stamps = self._stack(res_deblend, "output_images_mean")
        dist = np.array([[row["galaxy_distances_to_center_x"], row["galaxy_distances_to_center_y"]] for row in res_deblend],
                        dtype=np.float64)
        shifts = position_optimization_batch(self.field_image if field_image is None else field_image, stamps, dist,
                                             bound=3.0, ctx=self._ctx)
        col = np.empty(len(res_deblend), dtype=object)
        for i in range(len(res_deblend)):
            col[i] = np.array([shifts[i, 0], shifts[i, 1]], dtype=np.float64)
        res_deblend["shifts"] = col
        return res_deblend

    # -- one deblending pass -----------------------------------------------------------------------
    def deblend_field(self, galaxy_distances_to_center, cutout_images=None, optimise_positions=False,
                      epistemic_criterion=100.0, mse_criterion=100.0, field_image=None, on_device=False):
        """Deblend the galaxies at `galaxy_distances_to_center` (field_deblender.py:219-383).

        returns a np.recarray with, per deblended galaxy: cutout_images, output_images_mean, output_images_stddev,
        shifts, list_idx, galaxy_distances_to_center_x/_y, epistemic_uncertainty, passed_cuts
        (a dict of None entries when no galaxy could be extracted, as the reference does).

        Default path (the reference's call sequence extract_cutouts -> deblend, :260-274): ONE engine call
        (dv_infer_cutouts_keep) - the field goes to the GPU once, every chunk's cutouts are gathered and cast to float32
        there, straight into the network's input, mean and stddev come back through the pinned transfer ring, and the
        float64 `cutout_images` the recarray carries are assembled on the host from the field (they are copies of host
        data) while the GPU works.  Same numbers, bit for bit, as extract_cutouts followed by deblend.

        on_device=True (engine-specific): the whole chain - cutout gather, network, and the compositing that
        get_predicted_field / get_residual_field do afterwards - runs on the GPU in one engine call
        (dv_infer_cutouts_composite) and only the field-sized results come back: BASELINE configs[4]'s million cutouts are
        167 GB of mean and stddev stamps that no longer cross the host link.  The recarray then carries the per-galaxy
        scalars (list_idx, positions, shifts, passed_cuts, mse_center) but no stamp images, and get_predicted_field() /
        get_residual_field() return the fields composited on the GPU - the same sums in the same order, bit for bit, as
        compositing the stamps of the default path.  Needs integer positions, the object's own field and no caller-supplied
        cutouts (each raises with a message otherwise).

        epistemic_uncertainty_estimation=True (constructor): the 100 Monte-Carlo decodes per galaxy are a stage of the same
        engine call in both modes (dv_infer_fields_mc_keep / _mc_composite with one field) - they run on the
        encoder output of the deblending pass, with the seed that follows the pass's own.  The default path returns the
        recarray it always did, bit for bit; on_device=True composites `predicted_epistemic_field` on the GPU and adds the
        per-galaxy `epistemic_norm` the cut is taken on next to `mse_center`.
        """
        if optimise_positions:
            raise NotImplementedError("optimise_positions=True is not wired into deblend_field: call deblend_field() and then "
                                      "DeblendField.optimise_positions(), which fits the positions of all rows on the GPU "
                                      "(deblend_cutout/optimization.py)")
        if on_device:
            if isinstance(cutout_images, np.ndarray):
                raise ValueError("on_device=True cuts the stamps out of the field on the GPU; caller-supplied cutout_images "
                                 "need the default path")
            return self._deblend_field_on_device(galaxy_distances_to_center, mse_criterion, field_image, epistemic_criterion)
        eps_std = None                   # the Monte-Carlo std stamps, when the deblending call itself estimated them
        res_deblend = {"cutout_images": None, "output_images_mean": None, "output_images_stddev": None,
                       "shifts": None, "list_idx": None}
        if field_image is None:
            field_image = self.field_image
        field_image = np.asarray(field_image)
        field_size = field_image.shape[1]
        cs, nb = self.cutout_size, self.nb_of_bands

        if isinstance(cutout_images, np.ndarray):
            output_images_mean, dist = deblend(self.net, cutout_images, normalise=self.normalise)
            output_images_stddev = dist.stddev().numpy()
            list_idx = list(range(0, len(output_images_mean)))
            cutouts = cutout_images                  # rows of list_idx
        else:
            # extract_cutouts (extraction.py:4-43): which windows fit the field ...
            n = len(galaxy_distances_to_center)
            starts, ok = cutout_windows(field_size, galaxy_distances_to_center, cs) if n else (np.zeros((0, 2), np.int32), np.zeros(0, bool))
            if field_image.ndim != 4 or field_image.shape[3] != nb:
                ok[:] = False                        # the reference's slice assignment raises for every galaxy (caught, flagged)
            list_idx = [int(i) for i in np.nonzero(ok)[0]]
            if n and not ok.all():
                print("Some galaxies are too close from the border of the field to be considered here.")
            if list_idx == []:
                print("No galaxy deblended. End of the iterative procedure.")
                return res_deblend
            core = getattr(self.net, "_core", None)
            if core is None or getattr(core, "engine", None) is None or field_image.shape[1] != field_image.shape[2]:
                # a wrapped or plain-callable net (anything deblend() accepts), or a field that is not square (the fused
                # engine call gathers from square fields only): the reference's two steps as they stand,
                # extract_cutouts (extraction.py:4-43) then deblend(net, cutout_images[list_idx]) (:260-274)
                # (slices taken on the host: a window that fits field_size but not the shorter axis of a rectangular field
                # comes out truncated - the reference's assignment raises for it and the galaxy is flagged, :36-41)
                cut = [field_image[0, xs:xs + cs, ys:ys + cs] for xs, ys in starts[ok]]
                fits = [c.shape == (cs, cs, nb) for c in cut]
                if not all(fits):
                    if ok.all():
                        print("Some galaxies are too close from the border of the field to be considered here.")
                    list_idx = [i for i, f in zip(list_idx, fits) if f]
                    cut = [c for c, f in zip(cut, fits) if f]
                    if list_idx == []:
                        print("No galaxy deblended. End of the iterative procedure.")
                        return res_deblend
                cutouts = np.array(cut, dtype=np.float64)
                output_images_mean, dist = deblend(self.net, cutouts, normalise=self.normalise)
                output_images_stddev = dist.stddev().numpy()
            else:
                # ... and deblend(net, cutout_images[list_idx]) (deblender.py:18) on them, gathered on the GPU.  The
                # previous pass's recarray is let go first: its 16 bytes per pixel go back to the result-array pool
                # (engine._HostPool) and this call's arrays reuse them - unless the caller still holds that recarray
                self.res_deblend = None
                self._device_fields = None
                eng = core.engine
                eng.set_normalise(bool(self.normalise))
                try:
                    if self.epistemic_uncertainty_estimation:
                        # the deblending pass and, on its encoder output, the 100 decodes of the estimate below in one
                        # call: the two seeds deblend() and deblend_epistemic() would draw, in that order
                        seed = core.next_seed()
                        r = eng.infer_cutouts_mc_keep(field_image[0], starts[ok], seed=seed, mc_seed=core.next_seed(),
                                                      nsamples=100)
                        eps_std = r["epistemic"]
                    else:
                        r = eng.infer_cutouts_keep(field_image[0], starts[ok], seed=core.next_seed())
                finally:
                    eng.set_normalise(False)
                output_images_mean, output_images_stddev, cutouts = r["loc"], r["scale"], r["cutouts"]
        if list_idx == []:
            print("No galaxy deblended. End of the iterative procedure.")
            return res_deblend
        rows = cutouts if len(cutouts) == len(list_idx) else cutouts[list_idx]   # stamp of galaxy list_idx[i] in row i

        if self.epistemic_uncertainty_estimation:
            # reference: np.std(deblend(net, [cutout] * 100)[0], axis=0) per object (field_deblender.py:303-313)
            if eps_std is None:
                _, eps_std = deblend_epistemic(self.net, rows, n_samples=100, normalise=self.normalise)
            epistemic_uncertainty = [e.astype(np.float64) for e in eps_std]
            eps_norm = np.array([np.sum(e[:, :, 2]) for e in epistemic_uncertainty]) / \
                np.array([np.sum(m[:, :, 2]) for m in output_images_mean])
        else:
            epistemic_uncertainty = list(np.zeros((len(list_idx), cs, cs, nb)))
            eps_norm = np.zeros(len(list_idx))

        # the reference's per-galaxy loop (:320-352), over all galaxies at once: mse() of the centre 10 x 10 pixels
        c0, c1 = int(cs / 2) - 5, int(cs / 2) + 5

        def _center_mse(lo, hi):
            diff = rows[lo:hi, c0:c1, c0:c1] - output_images_mean[lo:hi, c0:c1, c0:c1]
            return np.mean(np.square(diff).reshape(len(diff), -1), axis=1)            # metrics.mse per galaxy

        n_gal = len(rows)
        if n_gal >= 4096:          # strided 10 x 10 windows out of 167-KB stamps: a few host threads (numpy drops the GIL)
            from concurrent.futures import ThreadPoolExecutor
            nthr = 8
            edges = [n_gal * k // nthr for k in range(nthr + 1)]
            with ThreadPoolExecutor(nthr) as ex:
                mse_center = np.concatenate(list(ex.map(lambda k: _center_mse(edges[k], edges[k + 1]), range(nthr))))
        else:
            mse_center = _center_mse(0, n_gal)
        passed_cuts = [bool(v) for v in ~((eps_norm > epistemic_criterion) | (mse_center > mse_criterion))]
        gx = [galaxy_distances_to_center[k][0] for k in list_idx]
        gy = [galaxy_distances_to_center[k][1] for k in list_idx]
        shifts = [np.array([0, 0]) for _ in list_idx]

        self.nb_of_detected_objects += [len(list(galaxy_distances_to_center))]
        self.nb_of_deblended_galaxies += [len(list_idx)]

        res_deblend["cutout_images"] = list(rows)
        res_deblend["output_images_mean"] = list(output_images_mean)
        res_deblend["output_images_stddev"] = list(output_images_stddev)
        res_deblend["shifts"] = shifts
        res_deblend["list_idx"] = list_idx
        res_deblend["galaxy_distances_to_center_x"] = gx
        res_deblend["galaxy_distances_to_center_y"] = gy
        res_deblend["epistemic_uncertainty"] = epistemic_uncertainty
        res_deblend["passed_cuts"] = passed_cuts
        self.res_deblend = _to_records(res_deblend)
        self._device_fields = None          # the composited fields of an earlier on-device pass belonged to ITS recarray
        return self.res_deblend

    def _deblend_field_on_device(self, galaxy_distances_to_center, mse_criterion, field_image, epistemic_criterion=100.0):
        # the reference's get_residual_field always subtracts from self.field_image (:60), whatever field the stamps were cut
        # from: the device-composited residual can only stand in for it when both are the same field
        if field_image is not None and field_image is not self.field_image and not (
                np.shape(field_image) == self.field_image.shape and np.array_equal(field_image, self.field_image)):
            raise ValueError("on_device=True composites the residual against the field it cuts the stamps from, which must be "
                             "the object's own field_image; a different field_image needs the default path")
        field = np.ascontiguousarray(self.field_image[0])
        F, cs = field.shape[0], self.cutout_size
        d = np.asarray(galaxy_distances_to_center, dtype=np.float64).reshape(-1, 2)
        starts, ok = cutout_windows(F, d, cs)
        list_idx = [int(i) for i in np.nonzero(ok)[0]]
        res = {"cutout_images": None, "output_images_mean": None, "output_images_stddev": None, "shifts": None,
               "list_idx": None}
        if not list_idx:
            print("No galaxy deblended. End of the iterative procedure.")
            return res                       # res_deblend and the fields that belong to it stay as they were (as the reference)
        if not ok.all():
            print("Some galaxies are too close from the border of the field to be considered here.")
        dd = d[ok]
        if not np.array_equal(dd, np.floor(dd)):
            raise ValueError("on_device=True places stamps at integer positions; fractional distances need the default path")
        # where get_predicted_field puts a stamp: padded at int((F - cs) / 2) and shifted by the distance to the centre
        # (field_deblender.py:128-160)
        places = (int((F - cs) / 2) + dd).astype(np.int64)
        core = self.net._core
        eng = core.engine
        eng.set_normalise(bool(self.normalise))
        try:
            if self.epistemic_uncertainty_estimation:
                seed = core.next_seed()          # the default path's order: deblending pass, then Monte Carlo
                out = eng.infer_cutouts_mc_composite(field, starts[ok], places, seed=seed, mc_seed=core.next_seed(),
                                                     nsamples=100)
            else:
                out = eng.infer_cutouts_composite(field, starts[ok], places, seed=core.next_seed())
        finally:
            eng.set_normalise(False)
        self.nb_of_detected_objects += [len(d)]
        self.nb_of_deblended_galaxies += [len(list_idx)]
        n = len(list_idx)
        cols = {"list_idx": list_idx, "shifts": [np.array([0, 0])] * n,
                "galaxy_distances_to_center_x": list(dd[:, 0]), "galaxy_distances_to_center_y": list(dd[:, 1]),
                "mse_center": list(out["mse_center"])}
        if self.epistemic_uncertainty_estimation:
            cols["epistemic_norm"] = list(out["eps_norm"])
            cols["passed_cuts"] = list(~((out["eps_norm"] > epistemic_criterion) | (out["mse_center"] > mse_criterion)))
        else:
            cols["passed_cuts"] = list(~(out["mse_center"] > mse_criterion))
        self.res_deblend = pd.DataFrame(cols).to_records(index=False)
        self._device_fields = (self.res_deblend, out)      # the fields and the recarray they belong to, set together
        return self.res_deblend


# -- many fields at once (engine-specific) -------------------------------------------------------
def batch_windows(field_size, galaxy_distances_to_center, cutout_size=59):
    """The windows of the galaxies of M fields as one list, for the many-field engine calls.

    galaxy_distances_to_center: M arrays (n_m, 2) of distances to the centre of each galaxy's own field.  Window validity is
    cutout_windows' (the reference's rule, extraction.py:26-41), field by field.  Returns (starts (N, 2) int32, field_ptr
    (M + 1,) int64, list_idx: M int64 arrays of the galaxies of each field that were kept, distances (N, 2) float64 of the
    kept galaxies): rows field_ptr[m]:field_ptr[m + 1] belong to field m, in the order of its list_idx."""
    starts, kept, dists = [], [], []
    field_ptr = np.zeros(len(galaxy_distances_to_center) + 1, dtype=np.int64)
    for m, d in enumerate(galaxy_distances_to_center):
        d = np.asarray(d, dtype=np.float64)
        if d.size == 0:
            d = d.reshape(0, 2)
        if d.ndim != 2 or d.shape[1] != 2:
            raise ValueError(f"field {m}: expected distances (n, 2), got {d.shape}")
        st, ok = cutout_windows(field_size, d, cutout_size) if len(d) else (np.zeros((0, 2), np.int32), np.zeros(0, bool))
        starts.append(st[ok])
        kept.append(np.nonzero(ok)[0].astype(np.int64))
        dists.append(d[ok])
        field_ptr[m + 1] = field_ptr[m] + int(ok.sum())
    cat = lambda parts, dt: np.concatenate(parts).astype(dt).reshape(-1, 2) if parts else np.zeros((0, 2), dt)
    return cat(starts, np.int32), field_ptr, kept, cat(dists, np.float64)


class DeblendFieldBatch:
    """DeblendField for M fields of one size: every pass is ONE engine call for the galaxies of all fields, so a survey of
    small fields runs the network in full chunks instead of one latency-bound call per field.  Per field the results are
    those of DeblendField on that field, for the noise rows its galaxies have in the call (galaxies are numbered over all
    fields, field after field).  The epistemic estimate is an option of the pass (deblend_fields(...,
    epistemic_uncertainty_estimation=True)), not of the object: the Monte-Carlo decodes of all fields run inside the same
    engine call, on the encoder output of the deblending pass.

    deblend_fields(..., optimise_positions=True) also fits every galaxy's sub-pixel shift - with on_device=True inside the
    same engine call, on stamps that stay on the GPU, the fields being composited there at the fitted positions (DESIGN.md
    section 7i).  One field is this class with M = 1: DeblendField.deblend_field(optimise_positions=True) stays
    unimplemented."""

    DEFAULT_COLUMNS = [("cutout_images", "O"), ("output_images_mean", "O"), ("output_images_stddev", "O"), ("shifts", "O"),
                       ("list_idx", "<i8"), ("galaxy_distances_to_center_x", "<f8"), ("galaxy_distances_to_center_y", "<f8"),
                       ("epistemic_uncertainty", "O"), ("passed_cuts", "?")]
    ON_DEVICE_COLUMNS = [("list_idx", "<i8"), ("shifts", "O"), ("galaxy_distances_to_center_x", "<f8"),
                         ("galaxy_distances_to_center_y", "<f8"), ("mse_center", "<f8"), ("passed_cuts", "?")]
    ON_DEVICE_EPISTEMIC_COLUMNS = ON_DEVICE_COLUMNS[:-1] + [("epistemic_norm", "<f8"), ("passed_cuts", "?")]

    @staticmethod
    def measure_columns(nb_of_bands):
        """What deblend_fields(measure=True) appends to every recarray: the catalogue of measure_stamps and the measured
        centroid as a distance to the field centre."""
        return ms.catalogue_dtype(nb_of_bands) + [("measured_distance_x", "<f8"), ("measured_distance_y", "<f8")]

    @staticmethod
    def measure_mc_columns(nb_of_bands):
        """What deblend_fields(measure_samples=S) appends behind measure_columns: the Monte-Carlo catalogue of
        measure_stamps_mc."""
        return ms.catalogue_mc_dtype(nb_of_bands)

    @staticmethod
    def blend_columns():
        """What deblend_fields(blendedness=True) appends behind measure_columns: the recarray of measure_blendedness."""
        return ms.blend_dtype()

    @staticmethod
    def psf_columns():
        """What deblend_fields(measure=True, psf=...) appends behind measure_columns: the recarray of measure_stamps_psf."""
        return ms.psf_dtype()

    @staticmethod
    def aperture_columns(nb_of_bands, n_radii, n_fractions):
        """What deblend_fields(measure=True, apertures=...) appends behind measure_columns: the recarray of
        measure_apertures."""
        return ms.aperture_dtype(nb_of_bands, n_radii, n_fractions)

    @staticmethod
    def aperture_data_columns(nb_of_bands, n_radii):
        """What deblend_fields(measure=True, apertures=..., aperture_data=True) appends behind aperture_columns: the recarray
        of measure_apertures_on_fields."""
        return ms.aperture_data_dtype(nb_of_bands, n_radii)

    @staticmethod
    def fit_flux_columns(nb_of_bands):
        """What deblend_fields(measure=True, fit_flux=True) appends behind measure_columns: the recarray of fit_fluxes."""
        return ms.fit_flux_dtype(nb_of_bands)

    @staticmethod
    def fit_sky_columns(nb_of_bands):
        """What deblend_fields(measure=True, fit_flux=True, fit_sky=0 or 1) appends behind the columns of the flux fit
        (fit_flux_columns, or fit_flux_weighted_columns with fit_weights): fit_sky and fit_sky_err."""
        return ms.fit_sky_dtype(nb_of_bands)

    @staticmethod
    def fit_nonneg_columns(nb_of_bands):
        """What deblend_fields(measure=True, fit_flux=True, fit_nonneg=True) appends behind every other column of the flux fit
        (fit_flux_columns or fit_flux_weighted_columns, then fit_sky_columns with fit_sky): fit_scale_free, flux_fit_free,
        fit_clamped and fit_dual."""
        return ms.fit_nonneg_dtype(nb_of_bands)

    @staticmethod
    def fit_groups_columns(nb_of_bands):
        """What deblend_fields(measure=True, fit_flux=True, fit_groups=True) appends behind the columns of the flux fit
        (fit_flux_columns, or fit_flux_weighted_columns with fit_weights): fit_group and fit_group_size."""
        return ms.fit_groups_dtype(nb_of_bands)

    @staticmethod
    def moments_data_columns(nb_of_bands):
        """What deblend_fields(measure=True, moments_data=True) appends behind measure_columns: the recarray of
        measure_moments_on_fields."""
        return ms.moments_data_dtype(nb_of_bands)

    @staticmethod
    def fit_flux_weighted_columns(nb_of_bands):
        """What deblend_fields(measure=True, fit_flux=True, fit_weights=W) appends behind measure_columns: the recarray of
        fit_fluxes_weighted - fit_flux_columns, then fit_chi2 and fit_npix."""
        return ms.fit_flux_weighted_dtype(nb_of_bands)

    def _psf_index(self, psf, psf_index, field_ptr):
        """(psf (K, ps, ps), index (N,)) of a deblend_fields(psf=...) call: one image for all galaxies, one per field (the
        index follows from field_ptr), or K images with the caller's index per galaxy - a flat (N,) array or a list of M
        arrays like the distances, rows of galaxies too close to the border already dropped."""
        psf = np.asarray(psf, dtype=np.float64)
        N, M = int(field_ptr[-1]), self.nb_of_fields
        if psf.ndim == 2:
            if psf_index is not None:
                raise ValueError("one PSF image (ps, ps) serves every galaxy: psf_index goes with a stack (K, ps, ps)")
            return psf[None], np.zeros(N, np.int32)
        if psf.ndim != 3:
            raise ValueError(f"expected a PSF image (ps, ps) or a stack (K, ps, ps), got {psf.shape}")
        if psf_index is None:
            if psf.shape[0] != M:
                raise ValueError(f"{psf.shape[0]} PSF images for {M} fields: without psf_index the stack holds one PSF per field")
            return psf, np.repeat(np.arange(M, dtype=np.int32), np.diff(field_ptr))
        if isinstance(psf_index, (list, tuple)):
            parts = [q for q in (np.asarray(q).reshape(-1) for q in psf_index) if q.size]   # (an empty field has no dtype to give)
            index = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        else:
            index = np.asarray(psf_index).reshape(-1)
        if index.shape != (N,) or index.dtype.kind not in "iu":
            raise ValueError(f"psf_index must give one integer per deblended galaxy ({N}), got {index.shape} {index.dtype}")
        return psf, index

    def __init__(self, net, field_images, cutout_size=59, nb_of_bands=6, normalise=False):
        """
        parameters:
            net: network used to deblend the fields
            field_images: the fields, shape (M, size, size, bands)
            cutout_size: size of the stamps
            nb_of_bands: number of filters in the images
            normalise: normalise the stamps before the network
        """
        f = np.array(field_images, dtype=np.float64, copy=True, order="C")
        if f.ndim != 4 or f.shape[1] != f.shape[2] or f.shape[3] != nb_of_bands:
            raise ValueError(f"expected fields (M, F, F, {nb_of_bands}), got {f.shape}")
        self.net = net
        self.field_images = f
        self.nb_of_fields = f.shape[0]
        self.field_size = f.shape[1]
        self.cutout_size = cutout_size
        self.nb_of_bands = nb_of_bands
        self.normalise = normalise
        self.nb_of_detected_objects = []
        self.nb_of_deblended_galaxies = []
        self.res_deblend = None
        self._ctx_obj = getattr(getattr(net, "_core", None), "ctx", None)
        self._device_fields = None      # (res_deblend list, fields composited on the GPU) of the last on-device pass
        self._epistemic_pass = None     # the res_deblend list of the last pass, if it estimated the epistemic uncertainty
        self.position_fit = None        # per field {objective, iters, status} of the last on-device pass that fitted positions
        self.psf_moments = None         # {psf_shape, psf_aux, psf_iters, psf_status} of the last pass that took a psf
        self.sky_fit = None             # {sky_coef (M, bands, q), sky_cov (M, bands, q, q), sky_status (M, bands, q), sky_npix
                                        # (M, bands)} of the last pass that fitted a sky (fit_sky): the per-field arrays of
                                        # Context.scene_fit_flux_sky, fields without galaxies included
        self.nonneg_fit = None          # {nonneg_iters, nonneg_status (M, bands)} of the last pass that constrained the flux fit
                                        # to amplitudes >= 0 (fit_nonneg): the per-field arrays of Context.scene_fit_flux_nonneg

    @property
    def _ctx(self):
        if self._ctx_obj is None:
            self._ctx_obj = E.default_context()
        return self._ctx_obj

    def _shifts_column(self, n):
        col = np.empty(n, dtype=object)
        for i in range(n):
            col[i] = np.array([0, 0])
        return col

    @staticmethod
    def _fitted_column(shifts):
        col = np.empty(len(shifts), dtype=object)
        for i in range(len(shifts)):
            col[i] = np.array([shifts[i, 0], shifts[i, 1]], dtype=np.float64)
        return col

    def deblend_fields(self, galaxy_distances_to_center=None, mse_criterion=100.0, on_device=False,
                       epistemic_uncertainty_estimation=False, epistemic_criterion=100.0, epistemic_samples=100, *,
                       measure=False, return_fields=True, measure_samples=0, blendedness=False,
                       psf=None, psf_index=None, apertures=None, flux_fractions=None, aperture_data=False,
                       sky_sigma=None, fit_flux=False, fit_groups=False, moments_data=False, moments_weights=None,
                       fit_weights=None, fit_nonneg=False, fit_sky=None, optimise_positions=False):
        """Deblend the galaxies of every field in one engine call.

        galaxy_distances_to_center: a list of M arrays (n_m, 2); None detects them first (detect_objects_batch).
        Returns a list of M recarrays (kept in self.res_deblend) with the columns DeblendField.deblend_field gives in the
        same mode: by default the stamps (dv_infer_fields_keep), with on_device=True the per-galaxy scalars and mse_center
        only, the fields being composited on the GPU (dv_infer_fields_composite; integer positions).  A field without a
        valid galaxy gets an empty recarray.

        epistemic_uncertainty_estimation=True: `epistemic_samples` more stochastic decodes of every galaxy run in the same
        call (dv_infer_fields_mc_keep / _mc_composite; two consecutive seeds: the pass, then the Monte-Carlo stage), and a
        galaxy whose normalised uncertainty sum(std[:, :, 2]) / sum(mean[:, :, 2]) exceeds `epistemic_criterion` fails the
        cuts, as in DeblendField.  By default the `epistemic_uncertainty` column carries the float64 std stamps; with
        on_device=True the std stamps are composited on the GPU (get_predicted_fields()["predicted_epistemic_fields"]) and
        the recarrays gain an `epistemic_norm` column.

        optimise_positions=True: every galaxy's sub-pixel shift is fitted within [-3, 3]^2 from zero and written to the
        `shifts` column as float64 np.array([sx, sy]).  With on_device=True the fit runs inside the same engine call on the
        stamps in device memory (dv_infer_fields_fit_composite), the fields are composited on the GPU at the fitted
        positions and self.position_fit holds, per field, the fit's {objective, iters, status}; by default the pass is
        followed by self.optimise_positions(), and the fields are composited on request from the stamps.

        measure=True: every galaxy's catalogue row - flux and flux_err per band, the adaptive moments row, col, Mrr, Mrc,
        Mcc of the r band with iters and status, the derived sigma, e1, e2 (debvader_amd.measure.measurement) - is appended
        to the recarrays, with the measured centroid as a distance to the field centre (measured_distance_x / _y, to
        compare with galaxy_distances_to_center_x / _y).  With on_device=True the measurement is a stage of the same
        engine call, on the stamps in device memory (dv_infer_fields_measure); by default the
        returned stamps are measured with measure_stamps.  return_fields=False (with on_device=True and measure=True
        only) is the catalogue-only call: no field is composited or downloaded, and get_predicted_fields() /
        get_residual_fields() raise.  The measurement is not available inside the position-fit and Monte-Carlo calls:
        measure=True with optimise_positions=True or epistemic_uncertainty_estimation=True raises.

        measure_samples=S > 0 (with measure=True and on_device=True, with or without return_fields): errors on the
        catalogue from the network's own Monte-Carlo decodes (dv_infer_fields_measure_mc).  S more
        stochastic decodes of every galaxy run in the same call (two consecutive seeds, as with the epistemic estimate: the
        pass, then the decodes), each is measured on the GPU, and the recarrays gain flux_mc_mean, flux_mc_std (per band)
        and <q>_mc_mean, <q>_mc_std for q in row, col, Mrr, Mrc, Mcc, sigma, e1, e2 over the n_ok samples whose
        measurement converged (measure_mc_columns).  The other columns and the fields are those of the same call without
        it.  It is not available with optimise_positions=True or epistemic_uncertainty_estimation=True either.

        blendedness=True (with measure=True and on_device=True, with or without return_fields): how much of the light
        under every galaxy's own weight belongs to its neighbours (dv_infer_fields_measure_blend).
        The recarrays gain blend_weight, blend_child, blend_model, blend_data, blend_npix, blendedness and
        blendedness_data (blend_columns; debvader_amd.measure.measurement.measure_blendedness describes them): sums under
        the Gaussian of the galaxy's adaptive moments over its stamp, the composited mean field and the observed field,
        taken on the GPU once the field's composite is complete.  The other columns and the fields are those of the same
        call without it.  It is not available with optimise_positions=True, epistemic_uncertainty_estimation=True or
        measure_samples.

        psf=... (with measure=True and on_device=True, with or without return_fields): PSF-corrected shapes by
        re-Gaussianization (dv_infer_fields_measure_psf).  psf is one float64 image (ps, ps) for all
        galaxies, a stack (M, ps, ps) with one PSF per field, or a stack (K, ps, ps) with psf_index - one integer per
        deblended galaxy, flat or as a list of M arrays - picking every galaxy's PSF.  The correction runs behind every
        chunk's measurement on the stamps in device memory; the recarrays gain psf_columns (regauss_row .. regauss_status,
        rho4, psf_index, psf_Mrr, psf_Mrc, psf_Mcc, psf_rho4 and the derived sigma_corr, e1_corr, e2_corr, resolution;
        debvader_amd.measure.measurement.measure_stamps_psf describes them) and self.psf_moments holds the PSFs' own rows.
        The other columns and the fields are those of the same call without it.  It is not available with blendedness,
        measure_samples, optimise_positions=True or epistemic_uncertainty_estimation=True.

        apertures=(R, ...) (with measure=True and on_device=True, with or without return_fields): aperture photometry
        (dv_infer_fields_measure_aper) behind every chunk's measurement on the stamps in device memory:
        the flux, its error and the area in up to 8 circles of the given radii in pixels about the measured centroid, the
        Kron radius and the flux in the Kron ellipse of the galaxy's own moments, and the radii that hold flux_fractions
        (up to 4, by default 0.2, 0.5 and 0.8) of that flux.  The recarrays gain aperture_columns (ap_flux, ap_flux_err,
        ap_area, flux_auto, flux_auto_err, kron_radius, rho_auto, auto_area, flux_rho, aper_flags, aper_status and the derived
        flux_radius, kron_a, kron_b, concentration; debvader_amd.measure.measurement.measure_apertures describes them).
        apertures=() gives the Kron columns alone.  The other columns and the fields are those of the same call without it.
        It is not available with psf, blendedness, measure_samples, optimise_positions=True or
        epistemic_uncertainty_estimation=True.

        aperture_data=True (with apertures, with or without return_fields): the same apertures on the observed field with
        the neighbours' models subtracted (dv_infer_fields_measure_aper_data).  Once a field's
        composite is complete, the sums of the composited mean field and of the observed field over every aperture - the
        stamp pixels inside the field, the same sub-pixel weights - are taken on the GPU; the recarrays gain
        aperture_data_columns (ap_model_sum, ap_data_sum, ap_field_area, auto_model_sum, auto_data_sum, auto_field_area and
        the derived ap_flux_data = ap_flux + ap_data_sum - ap_model_sum, flux_auto_data, ap_blendedness, auto_blendedness,
        aper_data_flags, ap_flux_data_err, flux_auto_data_err; debvader_amd.measure.measurement.measure_apertures_on_fields
        describes them).  sky_sigma, (bands,) or (M, bands), is the standard deviation of the sky per pixel the two error
        columns are derived from; without it they are NaN.  The other columns and the fields are those of the same call
        without it.

        fit_flux=True (with measure=True and on_device=True, with or without return_fields): the simultaneous flux fit of
        the deblended models to the observed field (dv_infer_fields_measure_fit).  The mean stamps are
        kept on the device, and once a field's composite is complete the amplitudes of all its galaxies are fitted to the
        observed pixels at once, per band, the shapes held fixed; the recarrays gain fit_flux_columns (fit_scale, fit_var,
        fit_gram, fit_proj, fit_status and the derived flux_fit = fit_scale * flux, fit_scale_alone, fit_independence,
        fit_scale_err, flux_fit_err; debvader_amd.measure.measurement.fit_fluxes describes them).  sky_sigma, (bands,) or (M,
        bands), is the standard deviation of the sky per pixel the two error columns are derived from; without it they are
        NaN.  The other columns and the fields are those of the same call without it.  It is not available with psf,
        apertures, blendedness, measure_samples, optimise_positions=True or epistemic_uncertainty_estimation=True.

        fit_weights=W (with fit_flux=True, with or without return_fields): the flux fit under per-pixel weights
        (dv_infer_fields_measure_fit_weighted).  W (M, F, F, bands) is the inverse variance of every pixel
        of the fields, 0 where a pixel is masked - any weight outside (0, inf) masks it, NaN included, and a NaN or saturated
        value of the field under a masked pixel reaches no sum.  The recarrays gain fit_flux_weighted_columns: those of
        fit_flux, with fit_scale_err = sqrt(fit_var) and flux_fit_err derived from the weights, then fit_chi2, the chi-square
        of the refitted scene under the galaxy's own counting pixels, and fit_npix, their number
        (debvader_amd.measure.measurement.fit_fluxes_weighted describes them).  sky_sigma beside fit_weights is
        refused: the weights already carry the noise.  It changes no other refusal of fit_flux.

        fit_sky=0 or 1 (with fit_flux=True, with or without fit_weights and return_fields): a sky background per field and
        band is fitted jointly with the amplitudes (dv_infer_fields_measure_fit_sky) - 0: a constant,
        1: a plane - to all pixels of the field (with fit_weights: the counting ones).  A sky residual under a blend then no
        longer goes into the amplitudes.  Beside fit_weights the fit runs with the weights.  The recarrays gain, behind the
        columns of fit_flux (and fit_chi2, fit_npix if weighted), fit_sky_columns: fit_sky, the fitted background at the
        centre pixel of the galaxy's stamp, and fit_sky_err (times sky_sigma unweighted, NaN without it;
        debvader_amd.measure.measurement.fit_fluxes_sky describes them).  fit_var and the errors derived from it now carry the
        covariance with the sky.  self.sky_fit holds the per-field arrays sky_coef, sky_cov, sky_status and sky_npix of the
        pass, fields without galaxies included.  Unweighted, a non-finite pixel anywhere in a field reaches every galaxy of
        that field through the sky: mask it with fit_weights.  It changes no other refusal of fit_flux.

        fit_nonneg=True (with fit_flux=True, with or without fit_weights, fit_sky and return_fields): the amplitudes of the
        flux fit are constrained to be >= 0, the sky left free (dv_infer_fields_measure_fit_nonneg).  A
        spurious or very faint detection under a brighter neighbour then gets exactly zero flux instead of a negative one, and
        the neighbour is no longer biased upwards by the light the negative model gave back.  In the columns of the flux fit
        fit_scale and flux_fit are 0 for a clamped galaxy and fit_var, fit_scale_err, flux_fit_err and fit_independence NaN;
        the recarrays gain, behind every other column, fit_nonneg_columns: fit_scale_free and flux_fit_free, the amplitude and
        flux of the fit without the constraint, fit_clamped and fit_dual (debvader_amd.measure.measurement.fit_fluxes_nonneg
        describes them).  self.nonneg_fit holds the per-field arrays nonneg_iters and nonneg_status of the pass.  A field and
        band without a negative amplitude keeps the values of the call without it.  It changes no other refusal of fit_flux.

        fit_groups=True (with fit_flux=True, with or without fit_weights, sky_sigma and return_fields): the flux fit is solved
        blend group by blend group (dv_infer_fields_measure_fit_groups) - the connected components of
        the graph of stamps whose rectangles, clipped to the field, intersect.  A field may then hold any number of galaxies
        (1024 per group), and the columns of the flux fit keep the bits of the fit without it wherever that one takes the
        field.  The recarrays gain, behind the columns of fit_flux (and fit_chi2, fit_npix if weighted), fit_groups_columns:
        fit_group, the smallest row of the galaxy's group in its field's recarray, and fit_group_size.  Together with fit_sky
        or fit_nonneg it is a ValueError: those two are not built for the grouped fit yet.

        moments_data=True (with measure=True and on_device=True, with or without return_fields): the adaptive moments
        re-measured on the observed field with the neighbours' models subtracted (dv_infer_fields_measure_moments_data,
        DESIGN.md section 7x).  The mean stamps are kept on the device, and once a field's composite is complete the child
        image of every galaxy - the observed pixels less the composited mean field plus the galaxy's own stamp - is measured as
        the mean stamp was; the recarrays gain moments_data_columns (flux_data, npix_data, row_data, col_data, Mrr_data,
        Mrc_data, Mcc_data, iters_data, status_data and the derived sigma_data, e1_data, e2_data, flux_data_err;
        debvader_amd.measure.measurement.measure_moments_on_fields describes them).  moments_weights=W (M, F, F, bands) is a
        mask: a pixel counts iff 0 < W < inf, elsewhere the galaxy's own model stands in.  sky_sigma, (bands,) or (M, bands),
        is the standard deviation of the sky per pixel flux_data_err is derived from; without it that column is NaN.  The other
        columns and the fields are those of the same call without it.  It is not available with any other extra, with
        optimise_positions=True or with epistemic_uncertainty_estimation=True."""
        mc = bool(epistemic_uncertainty_estimation)
        fit = bool(optimise_positions)
        measure = bool(measure)
        aperture_data, fit_flux, fit_nonneg, fit_groups = bool(aperture_data), bool(fit_flux), bool(fit_nonneg), bool(fit_groups)
        moments_data = bool(moments_data)
        band = 2                        # the band of the measurement (r): the engine call and the blendedness in the apertures
        kw = dict(measure_samples=measure_samples, blendedness=blendedness, psf=psf, psf_index=psf_index, apertures=apertures,
                  flux_fractions=flux_fractions, aperture_data=aperture_data, fit_flux=fit_flux, fit_weights=fit_weights,
                  fit_sky=fit_sky, fit_nonneg=fit_nonneg, fit_groups=fit_groups, moments_data=moments_data,
                  moments_weights=moments_weights)
        given = [x.key for x in _EXTRAS if x.given(kw[x.key])]
        if fit_groups and (fit_sky is not None or fit_nonneg):
            raise ValueError(ms.GROUPS_TAKE_NO_SKY_NO_CONSTRAINT)
        for x in _EXTRAS[1:]:           # (measure_samples, the oldest, is refused below its own integer check)
            _refuse_extra(x, kw, given, measure, on_device, fit, mc)
        if sky_sigma is not None and not aperture_data and not fit_flux and not moments_data:
            raise ValueError("sky_sigma is the sky noise of the data-flux errors of aperture_data=True: give aperture_data too")
        if fit_sky is not None:
            E.sky_terms(fit_sky)                                                                            # (ValueError)
        if fit_weights is not None:
            if sky_sigma is not None:
                raise ValueError(ms.WEIGHTS_CARRY_THE_NOISE)
            fit_weights = E.check_fit_weights(fit_weights, self.field_images.shape)                         # (ValueError)
        if moments_weights is not None:
            moments_weights = E.check_fit_weights(moments_weights, self.field_images.shape)                 # (ValueError)
        if sky_sigma is not None:
            sky_sigma = ms.check_sky_sigma(sky_sigma, self.nb_of_fields, self.nb_of_bands)                  # (ValueError)
        aper_par = None
        if apertures is not None:
            aper_par = E.aperture_params(apertures, (0.2, 0.5, 0.8) if flux_fractions is None else flux_fractions)   # (ValueError)
        if int(measure_samples) != measure_samples or int(measure_samples) < 0:
            raise ValueError(f"measure_samples must be an integer >= 0, got {measure_samples}")
        _refuse_extra(_EXTRAS[0], kw, given, measure, on_device, fit, mc)
        if measure and (fit or mc):
            raise ValueError("measure=True cannot be combined with optimise_positions=True or "
                             "epistemic_uncertainty_estimation=True: the measurement is a stage of the plain composite call "
                             "only (dv_infer_fields_measure), not of the position-fit or Monte-Carlo calls; run those passes "
                             "without it, or measure their stamps with debvader_amd.measure.measurement.measure_stamps")
        if not return_fields and not (measure and on_device):
            raise ValueError("return_fields=False is the catalogue-only call: it needs measure=True and on_device=True")
        if measure and self.nb_of_bands < 3:
            raise ValueError(f"the adaptive moments are taken on band 2 (r); these fields have {self.nb_of_bands} band(s)")
        if fit and self.nb_of_bands < 3:
            raise ValueError(f"the position fit uses band 2 (r); these fields have {self.nb_of_bands} band(s)")
        if mc:
            if int(epistemic_samples) < 1:
                raise ValueError(f"epistemic_samples must be at least 1, got {epistemic_samples}")
            if self.nb_of_bands < 3:
                raise ValueError("the normalised epistemic uncertainty is read from band 2, these fields have "
                                 f"{self.nb_of_bands} bands")
        if galaxy_distances_to_center is None:
            from debvader_amd.detect.detection import detect_objects_batch
            galaxy_distances_to_center = detect_objects_batch(self.field_images, ctx=self._ctx)
        if len(galaxy_distances_to_center) != self.nb_of_fields:
            raise ValueError(f"{self.nb_of_fields} fields but {len(galaxy_distances_to_center)} lists of galaxy distances")
        F, cs, nb = self.field_size, self.cutout_size, self.nb_of_bands
        starts, field_ptr, kept, dd = batch_windows(F, galaxy_distances_to_center, cs)
        n_det = [len(d) for d in galaxy_distances_to_center]
        if sum(len(k) for k in kept) != sum(n_det):
            print("Some galaxies are too close from the border of the field to be considered here.")
        if on_device and not np.array_equal(dd, np.floor(dd)):
            raise ValueError("on_device=True places stamps at integer positions; fractional distances need the default path")
        core = getattr(self.net, "_core", None)
        eng = getattr(core, "engine", None)
        if eng is None:
            raise ValueError("DeblendFieldBatch needs a net that runs on the engine (debvader_amd.model.model.load_deblender)")
        self.res_deblend = None
        self._device_fields = None
        self._epistemic_pass = None
        self.position_fit = None
        self.psf_moments = None
        self.sky_fit = None
        self.nonneg_fit = None
        N = len(starts)
        if psf is not None:
            psf, psf_index = self._psf_index(psf, psf_index, field_ptr)
        extras = [x for x in _EXTRAS if x.key in given]
        c = SimpleNamespace(bands=nb, band=band, sky_sigma=sky_sigma, field_ptr=field_ptr, psf=psf, psf_index=psf_index,
                            aper_par=aper_par, nmc=int(measure_samples), fit_weights=fit_weights, fit_sky=fit_sky,
                            moments_weights=moments_weights, places=(int((F - cs) / 2) + dd).astype(np.int64), cs=cs, F=F, core=core)
        eng.set_normalise(bool(self.normalise))
        try:
            seed = core.next_seed()
            if mc:
                mc_args = {"seed": seed, "mc_seed": core.next_seed(), "nsamples": int(epistemic_samples)}
            if on_device and fit:
                out = eng.infer_fields_fit_composite(self.field_images, starts, dd, field_ptr, bound=3.0,
                                                     **(mc_args if mc else {"seed": seed}))
            elif on_device:
                # where get_predicted_field puts a stamp: padded at int((F - cs) / 2) and shifted by the distance to the centre
                places = (int((F - cs) / 2) + dd).astype(np.int64)
                if mc:
                    out = eng.infer_fields_mc_composite(self.field_images, starts, places, field_ptr, **mc_args)
                elif measure:
                    # the plain measuring call, or the call of the one extra given (of the refining one where there are two)
                    x = extras[-1] if extras else None
                    call = getattr(eng, x.method if x else "infer_fields_measure")
                    out = call(self.field_images, starts, field_ptr,
                               places=places if return_fields or (x and x.places_always) else None, seed=seed,
                               **(x.kwargs(c) if x else {}), return_fields=bool(return_fields))
                else:
                    out = eng.infer_fields_composite(self.field_images, starts, places, field_ptr, seed=seed)
            elif mc:
                out = eng.infer_fields_mc_keep(self.field_images, starts, field_ptr, **mc_args)
            else:
                out = eng.infer_fields_keep(self.field_images, starts, field_ptr, seed=seed)
        finally:
            eng.set_normalise(False)
        eps_norm = None
        if mc and on_device:
            eps_norm = out["eps_norm"]
        elif mc:
            # DeblendField's host formula, row by row (float64 std stamps over numpy's float32 sum of the mean)
            eps64 = out["epistemic"].astype(np.float64)
            eps_norm = np.array([np.sum(e[:, :, 2]) for e in eps64]) / np.array([np.sum(m[:, :, 2]) for m in out["loc"]]) \
                if N else np.zeros(0)
        if on_device:
            mse_center = out["mse_center"]
        else:
            c0, c1 = int(cs / 2) - 5, int(cs / 2) + 5
            diff = out["cutouts"][:, c0:c1, c0:c1] - out["loc"][:, c0:c1, c0:c1]
            mse_center = np.mean(np.square(diff).reshape(N, -1), axis=1) if N else np.zeros(0)
            no_epistemic = np.zeros((cs, cs, nb))
            no_epistemic.flags.writeable = False          # one array stands for every row's zeros
        passed = ~(mse_center > mse_criterion) if eps_norm is None else \
            ~((eps_norm > epistemic_criterion) | (mse_center > mse_criterion))
        columns = self.DEFAULT_COLUMNS if not on_device else \
            self.ON_DEVICE_EPISTEMIC_COLUMNS if mc else self.ON_DEVICE_COLUMNS
        if measure:
            cat = ms.catalogue_records(out["flux"], out["flux_err"], out["shape"], out["iters"], out["status"]) if on_device \
                else ms.measure_stamps(out["loc"], out["scale"], ctx=self._ctx)
            columns = columns + self.measure_columns(nb)
            cats = [cat]
            for x in extras:
                columns = columns + x.columns(c)
                cats.append(x.records(out, c))
            if psf is not None:
                self.psf_moments = {k: out[k] for k in ("psf_shape", "psf_aux", "psf_iters", "psf_status")}
            if fit_sky is not None:
                self.sky_fit = {k: out[k] for k in E.FIT_SKY_KEYS}
            if fit_nonneg:
                self.nonneg_fit = {k: out[k] for k in E.FIT_NONNEG_FIELD_KEYS}
            # a stamp's pixel (row, col) is the field's pixel start + (row, col); distances count from pixel int(F / 2)
            measured = starts + np.stack([cat["row"], cat["col"]], axis=1) - int(F / 2) if N else np.zeros((0, 2))
        res = []
        for m in range(self.nb_of_fields):
            lo, hi = int(field_ptr[m]), int(field_ptr[m + 1])
            n = hi - lo
            rec = np.recarray((n,), dtype=columns)
            rec["list_idx"] = kept[m]
            rec["shifts"] = self._shifts_column(n) if not (on_device and fit) else self._fitted_column(out["shifts"][lo:hi])
            rec["galaxy_distances_to_center_x"] = dd[lo:hi, 0]
            rec["galaxy_distances_to_center_y"] = dd[lo:hi, 1]
            rec["passed_cuts"] = passed[lo:hi]
            if measure:
                for part in cats:
                    for k in part.dtype.names:
                        rec[k] = part[k][lo:hi]
                rec["measured_distance_x"] = measured[lo:hi, 0]
                rec["measured_distance_y"] = measured[lo:hi, 1]
            if on_device:
                rec["mse_center"] = mse_center[lo:hi]
                if mc:
                    rec["epistemic_norm"] = eps_norm[lo:hi]
            else:
                for i in range(n):
                    rec["cutout_images"][i] = out["cutouts"][lo + i]
                    rec["output_images_mean"][i] = out["loc"][lo + i]
                    rec["output_images_stddev"][i] = out["scale"][lo + i]
                    rec["epistemic_uncertainty"][i] = eps64[lo + i] if mc else no_epistemic
            res.append(rec)
        self.nb_of_detected_objects += [n_det]
        self.nb_of_deblended_galaxies += [[len(k) for k in kept]]
        self.res_deblend = res
        if on_device:
            self._device_fields = (res, out)
        if mc:
            self._epistemic_pass = res
        if fit and on_device:
            self.position_fit = [{k: out[k][int(field_ptr[m]):int(field_ptr[m + 1])].copy() for k in ("objective", "iters", "status")}
                                 for m in range(self.nb_of_fields)]
        elif fit:
            self.optimise_positions()
        return res

    def _own_device_fields(self):
        if self._device_fields is not None and self._device_fields[0] is self.res_deblend:
            return self._device_fields[1]
        return None

    def _stack(self, rec, key):
        if key not in rec.dtype.names:
            raise ValueError(f"these recarrays have no {key!r} column: they come from deblend_fields(on_device=True), whose "
                             "stamps stayed on the GPU; run the default path to work from stamps")
        return np.array([np.asarray(row[key], dtype=np.float64) for row in rec], dtype=np.float64).reshape(
            -1, self.cutout_size, self.cutout_size, self.nb_of_bands)

    def _need_pass(self):
        if self.res_deblend is None:
            raise ValueError("no deblend_fields() pass yet")

    @staticmethod
    def _need_fields(dev):
        if "mean_fields" not in dev:
            raise ValueError("the last pass was the catalogue-only call (deblend_fields(measure=True, return_fields=False)): it "
                             "composited no fields; run it with return_fields=True to get them")

    def get_residual_fields(self):
        """The fields minus every predicted galaxy at its position, (M, F, F, bands)."""
        self._need_pass()
        dev = self._own_device_fields()
        if dev is not None:
            self._need_fields(dev)
            return dev["residual_fields"].copy()
        out = self.field_images.copy()
        for m, rec in enumerate(self.res_deblend):
            if len(rec):
                out[m] = self._ctx.scene_composite(self.field_images[m], self._stack(rec, "output_images_mean"),
                                                   DeblendField._positions(rec), -1.0)
        return out

    def get_predicted_fields(self):
        """{"predicted_mean_fields", "predicted_stddev_fields"}, each (M, F, F, bands); after a pass that estimated the
        epistemic uncertainty also "predicted_epistemic_fields"."""
        self._need_pass()
        mc = self._epistemic_pass is not None and self._epistemic_pass is self.res_deblend
        dev = self._own_device_fields()
        if dev is not None:
            self._need_fields(dev)
            out = {"predicted_mean_fields": dev["mean_fields"].copy(), "predicted_stddev_fields": dev["stddev_fields"].copy()}
            if mc and "epistemic_fields" in dev:
                out["predicted_epistemic_fields"] = dev["epistemic_fields"].copy()
            return out
        out = {"predicted_mean_fields": np.zeros_like(self.field_images),
               "predicted_stddev_fields": np.zeros_like(self.field_images)}
        if mc:
            out["predicted_epistemic_fields"] = np.zeros_like(self.field_images)
        zeros = np.zeros(self.field_images.shape[1:])
        for m, rec in enumerate(self.res_deblend):
            if len(rec):
                pos = DeblendField._positions(rec)
                out["predicted_mean_fields"][m] = self._ctx.scene_composite(zeros, self._stack(rec, "output_images_mean"), pos)
                out["predicted_stddev_fields"][m] = self._ctx.scene_composite(zeros, self._stack(rec, "output_images_stddev"), pos)
                if mc:
                    out["predicted_epistemic_fields"][m] = self._ctx.scene_composite(
                        zeros, self._stack(rec, "epistemic_uncertainty"), pos)
        return out

    def optimise_positions(self):
        """Fit the sub-pixel shift of every row of every field in one engine call (position_optimization_fields) and write
        it to the `shifts` column, as DeblendField.optimise_positions does.  Returns the list of recarrays."""
        from debvader_amd.deblend_cutout.optimization import position_optimization_fields

        self._need_pass()
        res = self.res_deblend
        field_ptr = np.concatenate([[0], np.cumsum([len(r) for r in res])]).astype(np.int64)
        if field_ptr[-1] == 0:
            return res
        stamps = np.concatenate([self._stack(r, "output_images_mean") for r in res])
        dist = np.concatenate([np.stack([r["galaxy_distances_to_center_x"], r["galaxy_distances_to_center_y"]], axis=1)
                               for r in res]).astype(np.float64)
        shifts = position_optimization_fields(self.field_images, stamps, dist, field_ptr, bound=3.0, ctx=self._ctx)
        for m, rec in enumerate(res):
            rec["shifts"] = self._fitted_column(shifts[int(field_ptr[m]):int(field_ptr[m + 1])])
        self._device_fields = None
        return res
