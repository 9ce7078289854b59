"""Catalogue measurement of deblended galaxies: a flux and a shape per galaxy.

The reference ships `debvader.measure` as an empty package: measurement was meant to live there and was never written, so
there is no reference code behind this module.  The measurement itself is defined in DESIGN.md section 7j and runs on the
GPU (csrc/measure.hip): per-band fluxes and their errors summed over the network's mean / stddev stamps, and the adaptive
moments of one band - the centroid and second moments of the stamp under a Gaussian weight that is iterated until it matches
the object.  Errors on the centroid, the moments, sigma, e1 and e2 (and a second error on the fluxes) come from the network's
own Monte-Carlo decodes (measure_stamps_mc): every decode of a galaxy is measured and the measured
rows are folded into a mean and a standard deviation per quantity.  Blendedness - how much of the light under a galaxy's
own weight belongs to its neighbours - is DESIGN.md section 7l (measure_blendedness, csrc/blend.hip).  A PSF correction is not
part of it.
"""
import numpy as np

from debvader_amd import engine as E

STATUS_CONVERGED, STATUS_ITER_LIMIT, STATUS_FAILED = 0, 2, 3


def catalogue_dtype(nb_of_bands):
    """The columns of measure_stamps' recarray: what the GPU measures, then what the host derives from it."""
    nb = int(nb_of_bands)
    return [("flux", "<f8", (nb,)), ("flux_err", "<f8", (nb,)), ("row", "<f8"), ("col", "<f8"), ("Mrr", "<f8"),
            ("Mrc", "<f8"), ("Mcc", "<f8"), ("iters", "<i4"), ("status", "<i4"), ("sigma", "<f8"), ("e1", "<f8"),
            ("e2", "<f8")]


def catalogue_records(flux, flux_err, shape, iters, status):
    """The recarray of measure_stamps from the arrays the engine returns (flux_err None: NaN).  Derived on the host:
    sigma = det(M)^(1/4), e1 = (Mcc - Mrr) / (Mcc + Mrr), e2 = 2 Mrc / (Mcc + Mrr); NaN where status is 3."""
    flux = np.asarray(flux, dtype=np.float64)
    n, nb = flux.shape
    shape = np.asarray(shape, dtype=np.float64).reshape(n, 5)
    rec = np.recarray((n,), dtype=catalogue_dtype(nb))
    rec["flux"] = flux
    rec["flux_err"] = np.nan if flux_err is None else np.asarray(flux_err, dtype=np.float64)
    for k, name in enumerate(("row", "col", "Mrr", "Mrc", "Mcc")):
        rec[name] = shape[:, k]
    rec["iters"] = iters
    rec["status"] = status
    Mrr, Mrc, Mcc = shape[:, 2], shape[:, 3], shape[:, 4]
    failed = np.asarray(status) == STATUS_FAILED
    with np.errstate(all="ignore"):
        det, tr = Mrr * Mcc - Mrc * Mrc, Mcc + Mrr
        rec["sigma"] = np.where(failed, np.nan, np.sqrt(np.sqrt(det)))
        rec["e1"] = np.where(failed, np.nan, (Mcc - Mrr) / tr)
        rec["e2"] = np.where(failed, np.nan, 2.0 * Mrc / tr)
    return rec


MC_SHAPE_NAMES = E.MC_SHAPE_NAMES


def catalogue_mc_dtype(nb_of_bands):
    """The columns of measure_stamps_mc's recarray: mean and standard deviation over the Monte-Carlo decodes of the per-band
    fluxes (all samples) and of row, col, Mrr, Mrc, Mcc, sigma, e1, e2 (the n_ok accepted samples)."""
    nb = int(nb_of_bands)
    cols = [("flux_mc_mean", "<f8", (nb,)), ("flux_mc_std", "<f8", (nb,))]
    for q in MC_SHAPE_NAMES:
        cols += [(q + "_mc_mean", "<f8"), (q + "_mc_std", "<f8")]
    return cols + [("n_ok", "<i4")]


def catalogue_mc_records(flux_mc_mean, flux_mc_std, shape_mc_mean, shape_mc_std, n_ok):
    """The recarray of measure_stamps_mc from the arrays the engine returns."""
    flux_mc_mean = np.asarray(flux_mc_mean, dtype=np.float64)
    n, nb = flux_mc_mean.shape
    rec = np.recarray((n,), dtype=catalogue_mc_dtype(nb))
    rec["flux_mc_mean"] = flux_mc_mean
    rec["flux_mc_std"] = flux_mc_std
    for k, q in enumerate(MC_SHAPE_NAMES):
        rec[q + "_mc_mean"] = np.asarray(shape_mc_mean).reshape(n, 8)[:, k]
        rec[q + "_mc_std"] = np.asarray(shape_mc_std).reshape(n, 8)[:, k]
    rec["n_ok"] = n_ok
    return rec


def blend_dtype():
    """The columns of measure_blendedness' recarray: the four weighted sums and the pixel count the GPU takes, then the two
    ratios the host derives from them."""
    return [("blend_weight", "<f8"), ("blend_child", "<f8"), ("blend_model", "<f8"), ("blend_data", "<f8"),
            ("blend_npix", "<i4"), ("blendedness", "<f8"), ("blendedness_data", "<f8")]


def blend_records(blend, npix):
    """The recarray of measure_blendedness from the arrays the engine returns: blend (N, 4) = {W, A, Bm, Bd}, npix (N,).
    Derived on the host: blendedness = 1 - A / Bm, NaN where the row is ineligible (npix -1) or Bm <= 0;
    blendedness_data = 1 - A / Bd, NaN where the row is ineligible or Bd <= 0 (or no data field was given)."""
    blend = np.asarray(blend, dtype=np.float64).reshape(-1, 4)
    npix = np.asarray(npix)
    rec = np.recarray((blend.shape[0],), dtype=blend_dtype())
    for k, name in enumerate(("blend_weight", "blend_child", "blend_model", "blend_data")):
        rec[name] = blend[:, k]
    rec["blend_npix"] = npix
    A = blend[:, 1]
    with np.errstate(all="ignore"):
        for name, B in (("blendedness", blend[:, 2]), ("blendedness_data", blend[:, 3])):
            ok = (npix >= 0) & (B > 0)                       # (NaN > 0 is False)
            rec[name] = np.where(ok, 1.0 - A / np.where(ok, B, 1.0), np.nan)
    return rec


def residual_dtype():
    """The columns the iterative loop's end-of-loop sums add behind blend_dtype(): the two weighted
    sums the GPU takes over the final residual, then the two ratios the host derives from them."""
    return [("resid_sum", "<f8"), ("resid_sq", "<f8"), ("resid_mean", "<f8"), ("resid_rms", "<f8")]


def residual_records(weight, npix, resid_sum, resid_sq):
    """The recarray of residual_dtype() from W = sum g and npix (the child sums of a pass) and R1 = sum g final, R2 = sum g
    final^2 (FieldSet.blend_sums), all (N,).  Derived on the host: resid_mean = R1 / W, the mean of what the loop left under
    the galaxy's weight, and resid_rms = sqrt(R2 / W); both NaN where the row is ineligible (npix < 0) or W <= 0."""
    W = np.asarray(weight, dtype=np.float64).reshape(-1)
    npix = np.asarray(npix)
    R1, R2 = np.asarray(resid_sum, dtype=np.float64), np.asarray(resid_sq, dtype=np.float64)
    rec = np.recarray((W.shape[0],), dtype=residual_dtype())
    rec["resid_sum"] = R1
    rec["resid_sq"] = R2
    ok = (npix >= 0) & (W > 0)                               # (NaN > 0 is False)
    with np.errstate(all="ignore"):
        den = np.where(ok, W, 1.0)
        rec["resid_mean"] = np.where(ok, R1 / den, np.nan)
        rec["resid_rms"] = np.where(ok, np.sqrt(R2 / den), np.nan)
    return rec


def measure_blendedness(stamps_mean, catalogue, places, model_fields, data_fields=None, field_ptr=None, band=2, ctx=None):
    """Blendedness of N deblended galaxies on the GPU.

    parameters:
        stamps_mean: the network's mean stamps, (N, cutout_size, cutout_size, bands)
        catalogue: their measure_stamps recarray (row, col, Mrr, Mrc, Mcc and status are read), measured in `band`
        places: (N, 2), the field position (row, col) of every stamp's top-left corner - where the stamp was composited
        model_fields: (M, F, F, bands), the composited mean fields (the sum of all mean stamps of a field); (F, F, bands)
            for one field
        data_fields: the observed fields of the same shape, or None
        field_ptr: (M + 1,), stamps field_ptr[m]:field_ptr[m + 1] lie in field m; None: one field holds them all
        ctx: the engine context to run on (None: the default context)
    returns a np.recarray with, per galaxy, under the Gaussian weight g of its adaptive moments and over the stamp pixels
    that lie inside the field: blend_weight = sum g, blend_child = sum g * stamp, blend_model = sum g * model field,
    blend_data = sum g * data field (NaN without data_fields), blend_npix = the pixels summed, and, derived on the host,
    blendedness = 1 - blend_child / blend_model - the share of the neighbours in the model, 0 for a galaxy alone in its
    field - and blendedness_data = 1 - blend_child / blend_data, the same against the observed pixels (noisy, may be
    negative).  A galaxy whose measurement failed (status 3), or whose moments are not finite or have det M <= 1e-6, gets
    NaN and blend_npix = -1; a ratio whose denominator is not positive is NaN.
    """
    model = np.asarray(model_fields, dtype=np.float64)
    if model.ndim == 3:
        model = model[None]
        data_fields = None if data_fields is None else np.asarray(data_fields, dtype=np.float64)[None]
    shape = np.stack([np.asarray(catalogue[k], dtype=np.float64) for k in ("row", "col", "Mrr", "Mrc", "Mcc")], axis=1)
    if ctx is None:
        ctx = E.default_context()
    out = ctx.scene_blend(stamps_mean, shape, np.asarray(catalogue["status"], dtype=np.int32), places, model, data_fields,
                          field_ptr=field_ptr, band=band)
    return blend_records(out["blend"], out["npix"])


def measure_stamps_mc(samples, band=2, sigma0=3.0, tol=1e-10, max_iter=200, keep_samples=False, ctx=None):
    """Errors on the catalogue from Monte-Carlo decodes, on the GPU.

    parameters:
        samples: (S, N, cutout_size, cutout_size, bands) - S stochastic decodes (mean stamps) of each of N galaxies
        band, sigma0, tol, max_iter: as in measure_stamps; every sample is measured with them, without a stddev stamp
        keep_samples: also return the per-sample measurements
        ctx: the engine context to run on (None: the default context)
    returns a np.recarray with, per galaxy: flux_mc_mean, flux_mc_std (one entry per band, over all S samples) and
    <q>_mc_mean, <q>_mc_std for q in row, col, Mrr, Mrc, Mcc, sigma, e1, e2 over the n_ok samples whose measurement
    converged (status 0) with det M > 0 and a positive trace; n_ok = 0 gives NaN, n_ok = 1 a standard deviation of 0.  The
    standard deviations are the population form (np.std).  With keep_samples=True returns (recarray, {"sample_flux" (N, S,
    bands), "sample_shape" (N, S, 5), "sample_status" (N, S)}).
    """
    samples, _ = E.check_measure_mc_args(samples, band, sigma0, tol, max_iter)
    if ctx is None:
        ctx = E.default_context()
    out = ctx.scene_measure_mc(samples, band=band, sigma0=sigma0, tol=tol, max_iter=max_iter, keep_samples=bool(keep_samples))
    rec = catalogue_mc_records(out["flux_mc_mean"], out["flux_mc_std"], out["shape_mc_mean"], out["shape_mc_std"], out["n_ok"])
    if keep_samples:
        return rec, {k: out[k] for k in ("sample_flux", "sample_shape", "sample_status")}
    return rec


def measure_stamps(mean, stddev=None, band=2, sigma0=3.0, tol=1e-10, max_iter=200, ctx=None):
    """Measure N deblended galaxies on the GPU.

    parameters:
        mean: the network's mean stamps, (N, cutout_size, cutout_size, bands) - `output_images_mean` of a deblending pass
        stddev: its stddev stamps of the same shape (`output_images_stddev`), or None: `flux_err` is then NaN
        band: the band whose adaptive moments are taken (2, the r band)
        sigma0: width in pixels of the first Gaussian weight
        tol: the iteration stops when the centroid step (pixels) and the relative change of the moments are below it
        max_iter: iteration limit; 0 returns the initial state with status 2
        ctx: the engine context to run on (None: the default context)
    returns a np.recarray with, per galaxy: flux, flux_err (one entry per band), row, col (the centroid, in pixels from
    the stamp's pixel (0, 0)), Mrr, Mrc, Mcc (the adaptive second moments), iters, status (0 converged, 2 iteration limit,
    3 failed: degenerate moments, no positive weighted flux, or a centroid that left the stamp) and, derived on the host,
    sigma = det(M)^(1/4), e1 = (Mcc - Mrr) / (Mcc + Mrr), e2 = 2 Mrc / (Mcc + Mrr) - NaN where status is 3.
    """
    mean, stddev, _ = E.check_measure_args(mean, stddev, band, sigma0, tol, max_iter)
    if ctx is None:
        ctx = E.default_context()
    out = ctx.scene_measure(mean, stddev, band=band, sigma0=sigma0, tol=tol, max_iter=max_iter)
    return catalogue_records(out["flux"], out.get("flux_err"), out["shape"], out["iters"], out["status"])
