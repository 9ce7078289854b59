"""Catalogue measurement of deblended galaxies: a flux and a shape per galaxy.

The reference ships `debvader.measure` as an empty package: measurement was meant to live there and was never written, so
there is no reference code behind this module.  The measurement itself is defined in DESIGN.md section 7j and runs on the
GPU (csrc/measure.hip): per-band fluxes and their errors summed over the network's mean / stddev stamps, and the adaptive
moments of one band - the centroid and second moments of the stamp under a Gaussian weight that is iterated until it matches
the object.  Errors on the centroid, the moments, sigma, e1 and e2 (and a second error on the fluxes) come from the network's
own Monte-Carlo decodes (measure_stamps_mc): every decode of a galaxy is measured and the measured
rows are folded into a mean and a standard deviation per quantity.  Blendedness - how much of the light under a galaxy's
own weight belongs to its neighbours - is DESIGN.md section 7l (measure_blendedness, csrc/blend.hip).  The PSF correction
is DESIGN.md section 7n (measure_stamps_psf, csrc/regauss.hip): the re-Gaussianization of Hirata & Seljak (2003) - the part
of the galaxy's image that the PSF's departure from its own best-fitting Gaussian accounts for is taken off the stamp, the
adaptive moments of what remains are measured, and the PSF's moments are subtracted from them - which gives sigma_corr,
e1_corr, e2_corr and the resolution of every galaxy from a PSF image per galaxy, per field or for all.  Aperture photometry
is DESIGN.md section 7o (measure_apertures, csrc/aperture.hip): fluxes in fixed circular apertures about the measured
centroid, the Kron radius and the flux in the Kron ellipse of the galaxy's own moments (SExtractor's FLUX_AUTO and
KRON_RADIUS), and the radii that hold given fractions of that flux (FLUX_RADIUS).  The adaptive moments re-measured on the
observed field with the neighbours' models subtracted are DESIGN.md section 7x (measure_moments_on_fields,
csrc/moments_field.hip).
"""
import numpy as np

from debvader_amd import engine as E

STATUS_CONVERGED, STATUS_ITER_LIMIT, STATUS_FAILED = 0, 2, 3
# what the PSF correction adds (regauss_status): the catalogue row could not be used, no usable PSF, the galaxy is narrower
# than its PSF
STATUS_INELIGIBLE, STATUS_NO_PSF, STATUS_UNRESOLVED = 4, 5, 6


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
    rec["sigma"], rec["e1"], rec["e2"] = derived_shape(shape, status)
    return rec


def derived_shape(shape, status):
    """(sigma, e1, e2) of the adaptive-moments rows shape (N, 5) = {row, col, Mrr, Mrc, Mcc}: sigma = det(M)^(1/4), e1 = (Mcc -
    Mrr) / (Mcc + Mrr), e2 = 2 Mrc / (Mcc + Mrr); NaN where status is 3."""
    shape = np.asarray(shape, dtype=np.float64)
    Mrr, Mrc, Mcc = shape[:, 2], shape[:, 3], shape[:, 4]
    failed = np.asarray(status) == STATUS_FAILED
    with np.errstate(all="ignore"):
        det, tr = Mrr * Mcc - Mrc * Mrc, Mcc + Mrr
        return (np.where(failed, np.nan, np.sqrt(np.sqrt(det))), np.where(failed, np.nan, (Mcc - Mrr) / tr),
                np.where(failed, np.nan, 2.0 * Mrc / tr))


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


def psf_dtype():
    """The columns of measure_stamps_psf's recarray: the moments of the re-Gaussianized stamp and the galaxy's PSF the GPU
    measures, then what the host derives from them."""
    return [("regauss_row", "<f8"), ("regauss_col", "<f8"), ("regauss_Mrr", "<f8"), ("regauss_Mrc", "<f8"),
            ("regauss_Mcc", "<f8"), ("rho4", "<f8"), ("regauss_iters", "<i4"), ("regauss_status", "<i4"), ("psf_index", "<i4"),
            ("psf_Mrr", "<f8"), ("psf_Mrc", "<f8"), ("psf_Mcc", "<f8"), ("psf_rho4", "<f8"), ("sigma_corr", "<f8"),
            ("e1_corr", "<f8"), ("e2_corr", "<f8"), ("resolution", "<f8")]


def psf_records(regauss, regauss_iters, regauss_status, psf_shape, psf_aux, psf_index):
    """The recarray of measure_stamps_psf from the arrays the engine returns: regauss (N, 6) = {row', col', Mrr', Mrc', Mcc',
    rho4}, regauss_iters, regauss_status (N,), psf_shape (K, 5), psf_aux (K, 3) and the index (N,) of every galaxy's PSF.
    psf_Mrr, psf_Mrc, psf_Mcc and psf_rho4 are the rows of the galaxy's PSF (NaN for an index outside 0 .. K - 1).  Derived
    on the host from M_g = M' - M_P: sigma_corr = det(M_g)^(1/4), e1_corr = (Mcc - Mrr) / (Mcc + Mrr), e2_corr = 2 Mrc /
    (Mcc + Mrr), resolution = 1 - tr M_P / tr M'; the three shapes are NaN where regauss_status is 3 or above, det M_g <= 0
    or tr M_g <= 0, the resolution where regauss_status is 3 or above."""
    regauss = np.asarray(regauss, dtype=np.float64).reshape(-1, 6)
    n = regauss.shape[0]
    psf_shape = np.asarray(psf_shape, dtype=np.float64).reshape(-1, 5)
    psf_aux = np.asarray(psf_aux, dtype=np.float64).reshape(-1, 3)
    index = np.asarray(psf_index).reshape(n)
    status = np.asarray(regauss_status).reshape(n)
    rec = np.recarray((n,), dtype=psf_dtype())
    for k, name in enumerate(("regauss_row", "regauss_col", "regauss_Mrr", "regauss_Mrc", "regauss_Mcc", "rho4")):
        rec[name] = regauss[:, k]
    rec["regauss_iters"] = regauss_iters
    rec["regauss_status"] = status
    rec["psf_index"] = index
    known = (index >= 0) & (index < psf_shape.shape[0])
    safe = np.where(known, index, 0)
    P = np.where(known[:, None], psf_shape[safe, 2:5], np.nan) if psf_shape.shape[0] else np.full((n, 3), np.nan)
    rec["psf_Mrr"], rec["psf_Mrc"], rec["psf_Mcc"] = P[:, 0], P[:, 1], P[:, 2]
    rec["psf_rho4"] = np.where(known, psf_aux[safe, 2], np.nan) if psf_aux.shape[0] else np.nan
    with np.errstate(all="ignore"):
        Grr, Grc, Gcc = regauss[:, 2] - P[:, 0], regauss[:, 3] - P[:, 1], regauss[:, 4] - P[:, 2]
        det, tr = Grr * Gcc - Grc * Grc, Gcc + Grr
        ok = (status < STATUS_FAILED) & (det > 0) & (tr > 0)              # (NaN > 0 is False)
        rec["sigma_corr"] = np.where(ok, np.sqrt(np.sqrt(np.where(ok, det, 1.0))), np.nan)
        rec["e1_corr"] = np.where(ok, (Gcc - Grr) / np.where(ok, tr, 1.0), np.nan)
        rec["e2_corr"] = np.where(ok, 2.0 * Grc / np.where(ok, tr, 1.0), np.nan)
        rec["resolution"] = np.where(status < STATUS_FAILED, 1.0 - (P[:, 0] + P[:, 2]) / (regauss[:, 2] + regauss[:, 4]), np.nan)
    return rec


def measure_psf_moments(psf, psf_sigma0=2.0, tol=1e-10, max_iter=200, ctx=None):
    """The adaptive moments of PSF images on the GPU, as the PSF correction takes them.

    parameters:
        psf: (K, ps, ps) float64 PSF images, or one (ps, ps); they need not be normalised
        psf_sigma0: width in pixels of the first Gaussian weight
    returns {"psf_shape" (K, 5): {row, col, Mrr, Mrc, Mcc}, "psf_aux" (K, 3): {A_P - the amplitude of the best Gaussian -,
    the sum of the image, psf_rho4 - its kurtosis, 2 for a Gaussian}, "psf_iters", "psf_status" (K,)}.
    """
    if ctx is None:
        ctx = E.default_context()
    out = ctx.scene_regauss(np.zeros((0, 8, 8, 1), np.float32), np.zeros((0, 5)), np.zeros(0, np.int32), psf, band=0,
                            psf_sigma0=psf_sigma0, tol=tol, max_iter=max_iter)
    return {k: out[k] for k in ("psf_shape", "psf_aux", "psf_iters", "psf_status")}


def measure_stamps_psf(mean, psf, psf_index=None, catalogue=None, band=2, sigma0=3.0, tol=1e-10, max_iter=200, psf_sigma0=2.0,
                       ctx=None):
    """PSF-corrected shapes of N deblended galaxies on the GPU by re-Gaussianization.

    parameters:
        mean: the network's mean stamps, (N, cutout_size, cutout_size, bands)
        psf: (K, ps, ps) float64 PSF images in the stamps' pixel scale, or one (ps, ps) for all galaxies
        psf_index: (N,), the PSF of every galaxy; None: PSF 0
        catalogue: the measure_stamps recarray of the same stamps in `band` (row, col, Mrr, Mrc, Mcc and status are read);
            None: the stamps are measured first with band, sigma0, tol, max_iter
        psf_sigma0: width in pixels of the first Gaussian weight on the PSF images
        ctx: the engine context to run on (None: the default context)
    returns a np.recarray with, per galaxy: regauss_row, regauss_col, regauss_Mrr, regauss_Mrc, regauss_Mcc - the adaptive
    moments of the stamp less the part the PSF's departure from its best Gaussian accounts for -, rho4 - its kurtosis -,
    regauss_iters, regauss_status (0 converged, 2 iteration limit, 3 failed, 4 the catalogue row could not be used, 5 no
    usable PSF, 6 the galaxy is narrower than its PSF), psf_index, psf_Mrr, psf_Mrc, psf_Mcc, psf_rho4 - the moments of the
    galaxy's PSF - and, derived on the host from M_g = M' - M_P, sigma_corr, e1_corr, e2_corr and resolution = 1 - tr M_P /
    tr M' (psf_records).  rho4 and psf_rho4 are there for a caller that wants the fourth-order factor of Bernstein & Jarvis
    (2002) in the last step; the subtraction here is the plain one.
    """
    mean, _, _ = E.check_measure_args(mean, None, band, sigma0, tol, max_iter)
    if ctx is None:
        ctx = E.default_context()
    if catalogue is None:
        out = ctx.scene_measure(mean, None, band=band, sigma0=sigma0, tol=tol, max_iter=max_iter)
        shape, status = out["shape"], out["status"]
    else:
        shape = np.stack([np.asarray(catalogue[k], dtype=np.float64) for k in ("row", "col", "Mrr", "Mrc", "Mcc")], axis=1)
        status = np.asarray(catalogue["status"], dtype=np.int32)
    _, index = E.check_psf_args(psf, psf_index, mean.shape[0], psf_sigma0)
    out = ctx.scene_regauss(mean, shape, status, psf, index, band=band, psf_sigma0=psf_sigma0, tol=tol, max_iter=max_iter)
    return psf_records(out["regauss"], out["regauss_iters"], out["regauss_status"], out["psf_shape"], out["psf_aux"], index)


# aper_status of the aperture photometry: the catalogue row could not be used, no Kron radius (no positive flux inside
# kron_limit); aper_flags: bit k < 8 circle k is truncated by the stamp, then these
STATUS_NO_KRON = 7
APER_FLAG_AUTO_TRUNCATED, APER_FLAG_LIMIT_TRUNCATED, APER_FLAG_KRON_MIN = 1 << 8, 1 << 9, 1 << 10


def aperture_dtype(nb_of_bands, n_radii, n_fractions):
    """The columns of measure_apertures' recarray: what the GPU measures, then what the host derives from it."""
    nb, K, J = int(nb_of_bands), int(n_radii), int(n_fractions)
    return [("ap_flux", "<f8", (K, nb)), ("ap_flux_err", "<f8", (K, nb)), ("ap_area", "<f8", (K,)), ("flux_auto", "<f8", (nb,)),
            ("flux_auto_err", "<f8", (nb,)), ("kron_radius", "<f8"), ("rho_auto", "<f8"), ("auto_area", "<f8"),
            ("flux_rho", "<f8", (J,)), ("aper_flags", "<i4"), ("aper_status", "<i4"), ("flux_radius", "<f8", (J,)),
            ("kron_a", "<f8"), ("kron_b", "<f8"), ("concentration", "<f8")]


def aperture_records(ap_flux, ap_flux_err, ap_area, flux_auto, flux_auto_err, kron, flux_rho, aper_flags, aper_status, shape):
    """The recarray of measure_apertures from the arrays the engine returns (scene_aperture's, the two errors None without a
    stddev stamp: NaN) and shape (N, 5), the catalogue rows they were measured from.  kron_radius, rho_auto and auto_area are
    the three columns of kron.  Derived on the host, M = {Mrr, Mrc, Mcc} of shape: flux_radius = flux_rho det(M)^(1/4), the
    radii in circularised pixels; kron_a >= kron_b = rho_auto sqrt(lambda) with lambda the eigenvalues of M, the semi-axes of
    the automatic ellipse in pixels; concentration = 5 log10(flux_radius[J - 1] / flux_radius[0]) with at least two
    fractions.  NaN follows the GPU's: the three are NaN where aper_status is not 0, the concentration also with fewer than
    two fractions or a flux radius that is not positive."""
    flux_auto = np.asarray(flux_auto, dtype=np.float64)
    n, nb = flux_auto.shape
    ap_area = np.asarray(ap_area, dtype=np.float64).reshape(n, -1)
    flux_rho = np.asarray(flux_rho, dtype=np.float64).reshape(n, -1)
    K, J = ap_area.shape[1], flux_rho.shape[1]
    kron = np.asarray(kron, dtype=np.float64).reshape(n, 3)
    shape = np.asarray(shape, dtype=np.float64).reshape(n, 5)
    status = np.asarray(aper_status).reshape(n)
    rec = np.recarray((n,), dtype=aperture_dtype(nb, K, J))
    rec["ap_flux"] = np.asarray(ap_flux, dtype=np.float64).reshape(n, K, nb)
    rec["ap_flux_err"] = np.nan if ap_flux_err is None else np.asarray(ap_flux_err, dtype=np.float64).reshape(n, K, nb)
    rec["ap_area"] = ap_area
    rec["flux_auto"] = flux_auto
    rec["flux_auto_err"] = np.nan if flux_auto_err is None else np.asarray(flux_auto_err, dtype=np.float64)
    rec["kron_radius"], rec["rho_auto"], rec["auto_area"] = kron[:, 0], kron[:, 1], kron[:, 2]
    rec["flux_rho"] = flux_rho
    rec["aper_flags"] = aper_flags
    rec["aper_status"] = status
    Mrr, Mrc, Mcc = shape[:, 2], shape[:, 3], shape[:, 4]
    ok = status == 0
    with np.errstate(all="ignore"):
        det = Mrr * Mcc - Mrc * Mrc
        scale = np.where(ok, np.sqrt(np.sqrt(np.where(ok, det, 1.0))), np.nan)
        rec["flux_radius"] = flux_rho * scale[:, None]
        half, root = 0.5 * (Mrr + Mcc), np.sqrt(0.25 * (Mrr - Mcc) * (Mrr - Mcc) + Mrc * Mrc)
        rec["kron_a"] = np.where(ok, kron[:, 1] * np.sqrt(half + root), np.nan)
        rec["kron_b"] = np.where(ok, kron[:, 1] * np.sqrt(half - root), np.nan)
        if J >= 2:
            first, last = rec["flux_radius"][:, 0], rec["flux_radius"][:, J - 1]
            good = ok & (first > 0) & (last > 0)                    # (NaN > 0 is False)
            rec["concentration"] = np.where(good, 5.0 * np.log10(np.where(good, last, 1.0) / np.where(good, first, 1.0)), np.nan)
        else:
            rec["concentration"] = np.nan
    return rec


def measure_apertures(mean, stddev=None, catalogue=None, radii=(3.0, 5.0, 8.0), fractions=(0.2, 0.5, 0.8), band=2, sigma0=3.0,
                      tol=1e-10, max_iter=200, subsample=5, kron_factor=2.5, kron_min=3.5, kron_limit=6.0, bisect_iters=32,
                      ctx=None):
    """Aperture photometry of N deblended galaxies on the GPU.

    parameters:
        mean: the network's mean stamps, (N, cutout_size, cutout_size, bands)
        stddev: its stddev stamps (same shape); None: the two error columns are NaN
        catalogue: the measure_stamps recarray of the same stamps in `band` (row, col, Mrr, Mrc, Mcc and status are read);
            None: the stamps are measured first with band, sigma0, tol, max_iter
        radii: up to 8 radii in pixels of circular apertures about the measured centroid; () gives the Kron columns alone
        fractions: up to 4 fractions of flux_auto[band] whose radii are wanted (0.5: the half-light radius)
        subsample: a boundary pixel counts by the share of its subsample x subsample sub-pixel centres inside (1 .. 9)
        kron_factor, kron_min, kron_limit: the automatic ellipse has the radius max(kron_factor r1, kron_min) in units of the
            moment ellipse, r1 the first radial moment of the light inside kron_limit
        bisect_iters: halvings of [0, rho_auto] per flux radius
        ctx: the engine context to run on (None: the default context)
    returns a np.recarray with, per galaxy: ap_flux, ap_flux_err (K, bands), ap_area (K,), flux_auto, flux_auto_err (bands,),
    kron_radius (r1), rho_auto, auto_area, flux_rho (J,) in units of the moment ellipse, aper_flags (bit k: circle k is
    truncated by the stamp; APER_FLAG_AUTO_TRUNCATED, APER_FLAG_LIMIT_TRUNCATED, APER_FLAG_KRON_MIN), aper_status (0;
    STATUS_INELIGIBLE: the catalogue row could not be used, every float NaN; STATUS_NO_KRON: no positive flux inside
    kron_limit, the Kron columns NaN) and, derived on the host, flux_radius (J,) in circularised pixels, kron_a, kron_b - the
    semi-axes of the automatic ellipse in pixels - and concentration = 5 log10(flux_radius[J - 1] / flux_radius[0])
    (aperture_records).
    """
    mean, stddev, _ = E.check_measure_args(mean, stddev, band, sigma0, tol, max_iter)
    if ctx is None:
        ctx = E.default_context()
    if catalogue is None:
        out = ctx.scene_measure(mean, None, band=band, sigma0=sigma0, tol=tol, max_iter=max_iter)
        shape, status = out["shape"], out["status"]
    else:
        shape = np.stack([np.asarray(catalogue[k], dtype=np.float64) for k in ("row", "col", "Mrr", "Mrc", "Mcc")], axis=1)
        status = np.asarray(catalogue["status"], dtype=np.int32)
    out = ctx.scene_aperture(mean, shape, status, stddev, radii=radii, fractions=fractions, band=band, subsample=subsample,
                             kron_factor=kron_factor, kron_min=kron_min, kron_limit=kron_limit, bisect_iters=bisect_iters)
    return aperture_records(out["ap_flux"], out.get("ap_flux_err"), out["ap_area"], out["flux_auto"], out.get("flux_auto_err"),
                            out["kron"], out["flux_rho"], out["aper_flags"], out["aper_status"], shape)


# aper_data_flags of the apertures on the fields: bit k < 8 the field edge truncates circle k inside the stamp, then this
APER_DATA_FLAG_AUTO_TRUNCATED = 1 << 8


def aperture_data_dtype(nb_of_bands, n_radii):
    """The columns of measure_apertures_on_fields' recarray: what the GPU sums, then what the host derives from it."""
    nb, K = int(nb_of_bands), int(n_radii)
    return [("ap_model_sum", "<f8", (K, nb)), ("ap_data_sum", "<f8", (K, nb)), ("ap_field_area", "<f8", (K,)),
            ("auto_model_sum", "<f8", (nb,)), ("auto_data_sum", "<f8", (nb,)), ("auto_field_area", "<f8"),
            ("ap_flux_data", "<f8", (K, nb)), ("flux_auto_data", "<f8", (nb,)), ("ap_blendedness", "<f8", (K,)),
            ("auto_blendedness", "<f8"), ("aper_data_flags", "<i4"), ("ap_flux_data_err", "<f8", (K, nb)),
            ("flux_auto_data_err", "<f8", (nb,))]


def check_sky_sigma(sky_sigma, n_fields, nb_of_bands):
    """The per-band sky noise of the data-flux errors as (M, bands) float64: given as (bands,) for all fields or as (M,
    bands); every entry finite and positive."""
    sky = np.asarray(sky_sigma, dtype=np.float64)
    M, nb = int(n_fields), int(nb_of_bands)
    if sky.shape == (nb,):
        sky = np.broadcast_to(sky, (M, nb))
    elif sky.shape != (M, nb):
        raise ValueError(f"sky_sigma must have shape ({nb},) - one value per band - or ({M}, {nb}) - per field and band -, got "
                         f"{sky.shape}")
    if not np.all(np.isfinite(sky) & (sky > 0)):
        raise ValueError("sky_sigma must be finite and positive in every entry: it is the standard deviation of the sky noise "
                         "per pixel")
    return np.ascontiguousarray(sky)


def aperture_data_records(ap_model_sum, ap_data_sum, ap_field_area, auto_model_sum, auto_data_sum, auto_field_area, ap_flux,
                          ap_area, flux_auto, auto_area, band=2, sky_sigma=None, field_ptr=None):
    """The recarray of measure_apertures_on_fields from the six arrays the engine returns (scene_aperture_fields') and the
    columns ap_flux (N, K, bands), ap_area (N, K), flux_auto (N, bands), auto_area (N,) of the aperture photometry they go
    with.  Derived on the host: ap_flux_data = ap_flux + (ap_data_sum - ap_model_sum), the aperture on the observed field
    with the neighbours' models subtracted, and flux_auto_data likewise in the Kron ellipse; ap_blendedness = 1 -
    ap_flux[band] / ap_model_sum[band], the share of the neighbours in the model inside circle k (NaN where the denominator
    is not positive, exactly 0 for a galaxy alone in its field), auto_blendedness the same in the Kron ellipse;
    aper_data_flags: bit k < 8 where ap_field_area[k] != ap_area[k], APER_DATA_FLAG_AUTO_TRUNCATED where auto_field_area !=
    auto_area (a row whose areas are NaN sets no bit) - both are sums of whole numbers over the same s^2, so the comparison is
    exact; a set bit means the field edge
    truncates the aperture inside the stamp, and the model part of the data flux reaches further than its data part.  With
    sky_sigma (bands,) or (M, bands), the per-pixel standard deviation of the sky (field_ptr (M + 1,) gives every galaxy's
    field; None: one field): ap_flux_data_err = sky_sigma sqrt(ap_field_area), flux_auto_data_err likewise; without it the
    two are NaN.  NaN follows the GPU's."""
    auto_model_sum = np.asarray(auto_model_sum, dtype=np.float64)
    n, nb = auto_model_sum.shape
    ap_field_area = np.asarray(ap_field_area, dtype=np.float64)
    if ap_field_area.ndim != 2 or ap_field_area.shape[0] != n:
        raise ValueError(f"expected ap_field_area ({n}, K), got {ap_field_area.shape}")
    K = ap_field_area.shape[1]
    ap_model_sum = np.asarray(ap_model_sum, dtype=np.float64).reshape(n, K, nb)
    ap_data_sum = np.asarray(ap_data_sum, dtype=np.float64).reshape(n, K, nb)
    auto_data_sum = np.asarray(auto_data_sum, dtype=np.float64).reshape(n, nb)
    auto_field_area = np.asarray(auto_field_area, dtype=np.float64).reshape(n)
    ap_flux = np.asarray(ap_flux, dtype=np.float64).reshape(n, K, nb)
    ap_area = np.asarray(ap_area, dtype=np.float64).reshape(n, K)
    flux_auto = np.asarray(flux_auto, dtype=np.float64).reshape(n, nb)
    auto_area = np.asarray(auto_area, dtype=np.float64).reshape(n)
    if int(band) != band or not 0 <= int(band) < nb:
        raise ValueError(f"band {band} asked for, the sums have bands 0 .. {nb - 1}")
    band = int(band)
    rec = np.recarray((n,), dtype=aperture_data_dtype(nb, K))
    rec["ap_model_sum"], rec["ap_data_sum"], rec["ap_field_area"] = ap_model_sum, ap_data_sum, ap_field_area
    rec["auto_model_sum"], rec["auto_data_sum"], rec["auto_field_area"] = auto_model_sum, auto_data_sum, auto_field_area
    with np.errstate(all="ignore"):
        rec["ap_flux_data"] = ap_flux + (ap_data_sum - ap_model_sum)
        rec["flux_auto_data"] = flux_auto + (auto_data_sum - auto_model_sum)
        for name, child, model in (("ap_blendedness", ap_flux[:, :, band], ap_model_sum[:, :, band]),
                                   ("auto_blendedness", flux_auto[:, band], auto_model_sum[:, band])):
            ok = model > 0                                    # (NaN > 0 is False)
            rec[name] = np.where(ok, 1.0 - child / np.where(ok, model, 1.0), np.nan)
        flags = np.zeros(n, np.int32)
        for k in range(min(K, 8)):                            # (NaN areas - a row without apertures - set no bit)
            cut = np.isfinite(ap_field_area[:, k]) & np.isfinite(ap_area[:, k]) & (ap_field_area[:, k] != ap_area[:, k])
            flags |= np.where(cut, 1 << k, 0).astype(np.int32)
        cut = np.isfinite(auto_field_area) & np.isfinite(auto_area) & (auto_field_area != auto_area)
        flags |= np.where(cut, APER_DATA_FLAG_AUTO_TRUNCATED, 0).astype(np.int32)
        rec["aper_data_flags"] = flags
        if sky_sigma is None:
            rec["ap_flux_data_err"] = np.nan
            rec["flux_auto_data_err"] = np.nan
        else:
            if field_ptr is None:
                field_ptr = [0, n]
            fp = np.asarray(field_ptr, dtype=np.int64).reshape(-1)
            M = fp.shape[0] - 1
            if M < 1 or fp[0] != 0 or fp[-1] != n or (np.diff(fp) < 0).any():
                raise ValueError(f"field_ptr must start at 0, never decrease and end at the number of galaxies ({n})")
            sky = check_sky_sigma(sky_sigma, M, nb)[np.repeat(np.arange(M), np.diff(fp))]          # (N, bands)
            rec["ap_flux_data_err"] = sky[:, None, :] * np.sqrt(ap_field_area)[:, :, None]
            rec["flux_auto_data_err"] = sky * np.sqrt(auto_field_area)[:, None]
    return rec


def measure_apertures_on_fields(catalogue, places, model_fields, data_fields=None, field_ptr=None, sky_sigma=None,
                                apertures=None, radii=(3.0, 5.0, 8.0), cutout_size=59, subsample=5, band=2, ctx=None):
    """The aperture photometry of measure_apertures taken on the observed field with the neighbours' models subtracted, on the
    GPU: the sum over an aperture of D - T + P, D the observed field, T the composited mean field and
    P the galaxy's own stamp.  The sum over P is measure_apertures' ap_flux; the sums over T and D are taken here, over the
    pixels of the stamp that lie inside the field, with the same sub-pixel weights.

    parameters:
        catalogue: the measure_stamps recarray of the galaxies in `band` (row, col, Mrr, Mrc, Mcc and status are read) that
            also has the measure_apertures columns (ap_flux, ap_area, flux_auto, rho_auto, auto_area, aper_status) - as the
            recarrays of DeblendFieldBatch.deblend_fields(measure=True, apertures=...) do -, or `apertures` gives those
        places: (N, 2), the field position (row, col) of every stamp's top-left corner - where the stamp was composited
        model_fields: (M, F, F, bands), the composited mean fields (the sum of all mean stamps of a field); (F, F, bands)
            for one field
        data_fields: the observed fields of the same shape, or None: the data columns are NaN
        field_ptr: (M + 1,), galaxies field_ptr[m]:field_ptr[m + 1] lie in field m; None: one field holds them all
        sky_sigma: (bands,) or (M, bands), the standard deviation of the sky noise per pixel; None: the error columns are NaN
        apertures: the measure_apertures recarray of the same galaxies; None: its columns are read from `catalogue`
        radii, subsample: those the aperture photometry was taken with; cutout_size: the size of the stamps it was taken on
        ctx: the engine context to run on (None: the default context)
    returns a np.recarray with, per galaxy: ap_model_sum, ap_data_sum (K, bands), ap_field_area (K,), auto_model_sum,
    auto_data_sum (bands,), auto_field_area - the sums of w T, w D and w over the stamp pixels inside the field, in the K
    circles and in the Kron ellipse - and, derived on the host, ap_flux_data, flux_auto_data, ap_blendedness (K,),
    auto_blendedness, aper_data_flags, ap_flux_data_err and flux_auto_data_err (aperture_data_records).  A galaxy with
    aper_status STATUS_INELIGIBLE gets NaN, one with STATUS_NO_KRON NaN in the Kron columns.
    """
    model = np.asarray(model_fields, dtype=np.float64)
    if model.ndim == 3:
        model = model[None]
        data_fields = None if data_fields is None else np.asarray(data_fields, dtype=np.float64)[None]
    ap = catalogue if apertures is None else apertures
    missing = [k for k in ("row", "col", "Mrr", "Mrc", "Mcc", "status") if k not in catalogue.dtype.names] + \
        [k for k in ("ap_flux", "ap_area", "flux_auto", "kron_radius", "rho_auto", "auto_area", "aper_status") if k not in ap.dtype.names]
    if missing:
        raise ValueError(f"the catalogue lacks the columns {missing}: measure_apertures_on_fields takes the measure_stamps "
                         "columns and the measure_apertures columns of the same galaxies")
    radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    ap_flux = np.asarray(ap["ap_flux"], dtype=np.float64)
    if ap_flux.ndim != 3 or ap_flux.shape[1] != radii.size:
        raise ValueError(f"{radii.size} radii given, the catalogue's ap_flux has shape {ap_flux.shape}: give the radii the "
                         "aperture photometry was taken with")
    shape = np.stack([np.asarray(catalogue[k], dtype=np.float64) for k in ("row", "col", "Mrr", "Mrc", "Mcc")], axis=1)
    kron = np.stack([np.asarray(ap[k], dtype=np.float64) for k in ("kron_radius", "rho_auto", "auto_area")], axis=1)
    M = model.shape[0]
    if sky_sigma is not None:
        check_sky_sigma(sky_sigma, M, model.shape[-1])                   # (ValueError before any GPU work)
    if field_ptr is None and M == 1:
        field_ptr = [0, shape.shape[0]]
    if ctx is None:
        ctx = E.default_context()
    out = ctx.scene_aperture_fields(shape, np.asarray(catalogue["status"], dtype=np.int32), places, kron,
                                    np.asarray(ap["aper_status"], dtype=np.int32), model, data_fields, field_ptr=field_ptr,
                                    cutout_size=cutout_size, radii=radii, subsample=subsample)
    return aperture_data_records(out["ap_model_sum"], out["ap_data_sum"], out["ap_field_area"], out["auto_model_sum"],
                                 out["auto_data_sum"], out["auto_field_area"], ap_flux, ap["ap_area"], ap["flux_auto"],
                                 ap["auto_area"], band=band, sky_sigma=sky_sigma, field_ptr=field_ptr)


FIT_STATUS_INELIGIBLE, FIT_STATUS_DROPPED = 4, 5      # fit_status of the flux fit beside 0 (fitted)


def fit_flux_dtype(nb_of_bands):
    """The columns of fit_fluxes' recarray: what the GPU fits, then what the host derives from it."""
    nb = int(nb_of_bands)
    return [("fit_scale", "<f8", (nb,)), ("fit_var", "<f8", (nb,)), ("fit_gram", "<f8", (nb,)), ("fit_proj", "<f8", (nb,)),
            ("fit_status", "<i4", (nb,)), ("flux_fit", "<f8", (nb,)), ("fit_scale_alone", "<f8", (nb,)),
            ("fit_independence", "<f8", (nb,)), ("fit_scale_err", "<f8", (nb,)), ("flux_fit_err", "<f8", (nb,))]


def fit_flux_weighted_dtype(nb_of_bands):
    """The columns of fit_fluxes_weighted: fit_flux_dtype, then the chi-square of the refitted scene under the
    galaxy's own counting pixels and their number."""
    nb = int(nb_of_bands)
    return fit_flux_dtype(nb) + [("fit_chi2", "<f8", (nb,)), ("fit_npix", "<i4", (nb,))]


WEIGHTS_CARRY_THE_NOISE = ("sky_sigma cannot be given together with weights: the weights already carry the noise (they are the "
                           "inverse variance of every pixel, and fit_scale_err = sqrt(fit_var) follows from them); a uniform sky "
                           "is weight_fields = 1 / sky_sigma**2 broadcast to the fields")


def fit_flux_records(fit_scale, fit_var, fit_gram, fit_proj, fit_status, flux, sky_sigma=None, field_ptr=None, fit_chi2=None,
                     fit_npix=None, weighted=False):
    """The recarray of fit_fluxes from the five arrays the engine returns (scene_fit_flux's, all (N, bands)) and the stamp
    fluxes `flux` (N, bands) of the catalogue they go with.  Derived on the host: flux_fit = fit_scale * flux, the flux of
    the galaxy with the amplitude the observed pixels ask for; fit_scale_alone = fit_proj / fit_gram, the amplitude with the
    neighbours ignored (NaN where fit_gram is not positive); fit_independence = 1 / sqrt(fit_var * fit_gram), in (0, 1]: the
    ratio of the error of the amplitude with the neighbours held fixed to its error in the joint fit, 1 for a galaxy that
    overlaps nobody, small where two models can hardly be told apart.  With sky_sigma (bands,) or (M, bands), the per-pixel
    standard deviation of the sky (field_ptr (M + 1,) gives every galaxy's field; None: one field): fit_scale_err = sky_sigma
    sqrt(fit_var) and flux_fit_err = fit_scale_err |flux|; without it the two are NaN.  NaN follows the GPU's: an ineligible
    galaxy (fit_status 4) is NaN in every derived column of that band; a dropped one (5) has fit_scale 1, so flux_fit = flux,
    and NaN independence and errors.
    weighted=True (the arrays of a weighted fit): the weights were the inverse variance of every pixel, so
    fit_var is the variance of fit_scale - fit_scale_err = sqrt(fit_var) and flux_fit_err = fit_scale_err |flux|, and sky_sigma
    beside them is a ValueError.  With fit_chi2 and fit_npix (N, bands) too the recarray has fit_flux_weighted_dtype."""
    weighted = bool(weighted) or fit_chi2 is not None or fit_npix is not None
    if weighted and sky_sigma is not None:
        raise ValueError(WEIGHTS_CARRY_THE_NOISE)
    if (fit_chi2 is None) != (fit_npix is None):
        raise ValueError("fit_chi2 and fit_npix go together (both given or both None)")
    fit_scale = np.asarray(fit_scale, dtype=np.float64)
    if fit_scale.ndim != 2:
        raise ValueError(f"expected fit_scale (N, bands), got {fit_scale.shape}")
    n, nb = fit_scale.shape
    fit_var = np.asarray(fit_var, dtype=np.float64).reshape(n, nb)
    fit_gram = np.asarray(fit_gram, dtype=np.float64).reshape(n, nb)
    fit_proj = np.asarray(fit_proj, dtype=np.float64).reshape(n, nb)
    fit_status = np.asarray(fit_status, dtype=np.int32).reshape(n, nb)
    flux = np.asarray(flux, dtype=np.float64)
    if flux.shape != (n, nb):
        raise ValueError(f"expected flux ({n}, {nb}), got {flux.shape}")
    rec = np.recarray((n,), dtype=fit_flux_dtype(nb) if fit_chi2 is None else fit_flux_weighted_dtype(nb))
    rec["fit_scale"], rec["fit_var"], rec["fit_gram"], rec["fit_proj"] = fit_scale, fit_var, fit_gram, fit_proj
    rec["fit_status"] = fit_status
    if fit_chi2 is not None:
        rec["fit_chi2"] = np.asarray(fit_chi2, dtype=np.float64).reshape(n, nb)
        rec["fit_npix"] = np.asarray(fit_npix, dtype=np.int32).reshape(n, nb)
    with np.errstate(all="ignore"):
        rec["flux_fit"] = fit_scale * flux
        ok = fit_gram > 0                                     # (NaN > 0 is False)
        rec["fit_scale_alone"] = np.where(ok, fit_proj / np.where(ok, fit_gram, 1.0), np.nan)
        rec["fit_independence"] = 1.0 / np.sqrt(fit_var * fit_gram)
        if weighted:
            rec["fit_scale_err"] = np.sqrt(fit_var)
            rec["flux_fit_err"] = rec["fit_scale_err"] * np.abs(flux)
        elif sky_sigma is None:
            rec["fit_scale_err"] = np.nan
            rec["flux_fit_err"] = np.nan
        else:
            if field_ptr is None:
                field_ptr = [0, n]
            fp = np.asarray(field_ptr, dtype=np.int64).reshape(-1)
            M = fp.shape[0] - 1
            if M < 1 or fp[0] != 0 or fp[-1] != n or (np.diff(fp) < 0).any():
                raise ValueError(f"field_ptr must start at 0, never decrease and end at the number of galaxies ({n})")
            sky = check_sky_sigma(sky_sigma, M, nb)[np.repeat(np.arange(M), np.diff(fp))]          # (N, bands)
            rec["fit_scale_err"] = sky * np.sqrt(fit_var)
            rec["flux_fit_err"] = rec["fit_scale_err"] * np.abs(flux)
    return rec


def fit_fluxes(stamps_mean, places, data_fields, field_ptr=None, catalogue=None, sky_sigma=None, min_pivot=1e-8, ctx=None):
    """Simultaneous flux fit of N deblended galaxies to the observed fields on the GPU: the shapes of
    the galaxies of a field are held fixed at the network's mean stamps and all their amplitudes are fitted to the observed
    pixels at once, per band, by linear least squares - the flux re-fit of the SDSS deblender, the Tractor and scarlet.  A bias
    of the network on any member of a blend does not bias the fitted fluxes of the others.  Every pixel of a band has the same
    weight here; fit_fluxes_weighted takes a variance plane and a mask.

    parameters:
        stamps_mean: the network's mean stamps, (N, cutout_size, cutout_size, bands)
        places: (N, 2), the field position (row, col) of every stamp's top-left corner - where the stamp was composited
        data_fields: (M, F, F, bands), the observed fields; (F, F, bands) for one field
        field_ptr: (M + 1,), stamps field_ptr[m]:field_ptr[m + 1] lie in field m; None: one field holds them all
        catalogue: the measure_stamps recarray of the galaxies (its flux is read); None: the stamp flux is summed here, the
            float64 sum of every band of stamps_mean
        sky_sigma: (bands,) or (M, bands), the standard deviation of the sky noise per pixel; None: the error columns are NaN
        min_pivot: the relative Cholesky pivot under which a galaxy is dropped from the fit, in (0, 1)
        ctx: the engine context to run on (None: the default context)
    returns a np.recarray with, per galaxy and band: fit_scale, fit_var, fit_gram, fit_proj, fit_status (scene_fit_flux
    describes them) and, derived on the host, flux_fit, fit_scale_alone, fit_independence, fit_scale_err and flux_fit_err
    (fit_flux_records).  fit_status FIT_STATUS_INELIGIBLE: the stamp is zero or wholly outside the field in that band;
    FIT_STATUS_DROPPED: the galaxy cannot be told from the earlier galaxies of its field and keeps the network's amplitude.
    """
    return _fit_fluxes(stamps_mean, places, data_fields, None, field_ptr, catalogue, sky_sigma, min_pivot, ctx)


def fit_fluxes_weighted(stamps_mean, places, data_fields, weight_fields, field_ptr=None, catalogue=None, sky_sigma=None,
                        min_pivot=1e-8, ctx=None):
    """fit_fluxes under per-pixel inverse-variance weights, with masks and a chi-square.

    parameters: those of fit_fluxes, and
        weight_fields: the inverse variance of every pixel, of the shape of data_fields ((F, F, bands) for one field), 0 where
            a pixel is masked.  A pixel counts iff 0 < W < inf: any other weight masks it, NaN included, and nothing under a
            masked pixel - a NaN or a saturated value of the field - is read into a sum.  The values are not validated on the
            host; only the shape is, before any GPU work
        sky_sigma: must stay None - the weights already carry the noise; anything else is a ValueError
    returns a np.recarray of fit_flux_weighted_dtype: the columns of fit_fluxes, where fit_gram = sum W P^2, fit_proj = sum W P D
    over the counting pixels, fit_var is the variance of fit_scale, fit_scale_err = sqrt(fit_var) and flux_fit_err =
    fit_scale_err |flux|; then fit_chi2, the sum of W (D - model)^2 over the galaxy's own counting pixels with the model the
    refitted scene (NaN where the galaxy is FIT_STATUS_INELIGIBLE - no counting pixel, or a zero stamp), and fit_npix, the
    number of those pixels.  A user with a uniform sky passes weight_fields = 1 / sky_sigma**2 broadcast to the fields.
    """
    if weight_fields is None:
        raise ValueError("weight_fields must be given: fit_fluxes is the unweighted fit")
    return _fit_fluxes(stamps_mean, places, data_fields, weight_fields, field_ptr, catalogue, sky_sigma, min_pivot, ctx)


def _fit_fluxes(stamps_mean, places, data_fields, weight_fields, field_ptr, catalogue, sky_sigma, min_pivot, ctx):
    """The body fit_fluxes and fit_fluxes_weighted share (weight_fields None: the unweighted fit)"""
    data = np.asarray(data_fields, dtype=np.float64)
    if data.ndim == 3:
        data = data[None]
    M = data.shape[0]
    if weight_fields is not None:
        if sky_sigma is not None:
            raise ValueError(WEIGHTS_CARRY_THE_NOISE)
        weight_fields = E.check_fit_weights(weight_fields, data.shape)   # (ValueError before any GPU work)
    if data.ndim == 4 and sky_sigma is not None:
        check_sky_sigma(sky_sigma, M, data.shape[-1])                    # (ValueError before any GPU work)
    stamps = np.asarray(stamps_mean, dtype=np.float32)
    if field_ptr is None and M == 1:
        field_ptr = [0, stamps.shape[0]]
    if catalogue is None:
        flux = stamps.sum(axis=(1, 2), dtype=np.float64) if stamps.ndim == 4 else None
    else:
        if "flux" not in catalogue.dtype.names:
            raise ValueError("the catalogue lacks the column flux: fit_fluxes takes the measure_stamps recarray of the galaxies")
        flux = np.asarray(catalogue["flux"], dtype=np.float64)
    if ctx is None:
        ctx = E.default_context()
    if weight_fields is not None:
        out = ctx.scene_fit_flux(stamps, places, data, field_ptr=field_ptr, min_pivot=min_pivot, weight_fields=weight_fields)
        return fit_flux_records(*(out[k] for k in E.FIT_FLUX_KEYS), flux, field_ptr=field_ptr, fit_chi2=out["fit_chi2"],
                                fit_npix=out["fit_npix"])
    out = ctx.scene_fit_flux(stamps, places, data, field_ptr=field_ptr, min_pivot=min_pivot)
    return fit_flux_records(out["fit_scale"], out["fit_var"], out["fit_gram"], out["fit_proj"], out["fit_status"], flux,
                            sky_sigma=sky_sigma, field_ptr=field_ptr)


GROUPS_TAKE_NO_SKY_NO_CONSTRAINT = ("fit_groups=True cannot be combined with fit_sky or fit_nonneg: those two are not built for the "
                                    "grouped fit yet (the sky couples all groups of a field, and the non-negative fit reports per "
                                    "field and band)")


def fit_groups_dtype(nb_of_bands):
    """The two columns a flux fit by blend groups adds per galaxy; they do not depend on the band."""
    int(nb_of_bands)
    return [("fit_group", "<i4"), ("fit_group_size", "<i4")]


def fit_groups_records(fit_group, fit_group_size):
    """The recarray of fit_groups_dtype from the two arrays (N,) of scene_fit_flux_groups: fit_group, the smallest row of the
    galaxy's blend group counted from the first row of its field, and fit_group_size, the members of that group."""
    group = np.asarray(fit_group, dtype=np.int32)
    size = np.asarray(fit_group_size, dtype=np.int32)
    if group.ndim != 1 or size.shape != group.shape:
        raise ValueError(f"expected fit_group and fit_group_size (N,), got {group.shape} and {size.shape}")
    rec = np.recarray(group.shape, dtype=fit_groups_dtype(1))
    rec["fit_group"], rec["fit_group_size"] = group, size
    return rec


def fit_fluxes_groups(stamps_mean, places, data_fields, field_ptr=None, catalogue=None, sky_sigma=None, weights=None,
                      min_pivot=1e-8, ctx=None):
    """fit_fluxes, or fit_fluxes_weighted with `weights`, solved blend group by blend group on the GPU:
    the connected components of the graph of stamps whose rectangles, clipped to their field, intersect are found on the GPU
    and each is fitted on its own.  A field may hold any number of galaxies; a group of more than 1024 is refused.

    parameters: those of fit_fluxes, and
        weights: the weight fields of fit_fluxes_weighted, or None: the unweighted fit; with them sky_sigma must stay None
    returns a np.recarray of the columns of fit_fluxes (of fit_fluxes_weighted with weights) - the same bits wherever that
    call takes the field - and then fit_group, the smallest row of the galaxy's group counted from the first row of its field,
    and fit_group_size, the members of that group (fit_groups_dtype)."""
    data = np.asarray(data_fields, dtype=np.float64)
    if data.ndim == 3:
        data = data[None]
    M = data.shape[0]
    if weights is not None:
        if sky_sigma is not None:
            raise ValueError(WEIGHTS_CARRY_THE_NOISE)
        weights = E.check_fit_weights(weights, data.shape)                   # (ValueError before any GPU work)
    if data.ndim == 4 and sky_sigma is not None:
        check_sky_sigma(sky_sigma, M, data.shape[-1])                        # (ValueError before any GPU work)
    stamps = np.asarray(stamps_mean, dtype=np.float32)
    if field_ptr is None and M == 1:
        field_ptr = [0, stamps.shape[0]]
    if catalogue is None:
        flux = stamps.sum(axis=(1, 2), dtype=np.float64) if stamps.ndim == 4 else None
    else:
        if "flux" not in catalogue.dtype.names:
            raise ValueError("the catalogue lacks the column flux: fit_fluxes_groups takes the measure_stamps recarray of the galaxies")
        flux = np.asarray(catalogue["flux"], dtype=np.float64)
    if ctx is None:
        ctx = E.default_context()
    out = ctx.scene_fit_flux_groups(stamps, places, data, field_ptr=field_ptr, min_pivot=min_pivot, weight_fields=weights)
    if weights is not None:
        fit = fit_flux_records(*(out[k] for k in E.FIT_FLUX_KEYS), flux, field_ptr=field_ptr, fit_chi2=out["fit_chi2"],
                               fit_npix=out["fit_npix"])
    else:
        fit = fit_flux_records(*(out[k] for k in E.FIT_FLUX_KEYS), flux, sky_sigma=sky_sigma, field_ptr=field_ptr)
    return _join_records(fit, fit_groups_records(out["fit_group"], out["fit_group_size"]))


def _join_records(*recs):
    """One recarray with the columns of several of the same length, in their order"""
    out = np.recarray((len(recs[0]),), dtype=[d for r in recs for d in r.dtype.descr])
    for r in recs:
        for k in r.dtype.names:
            out[k] = r[k]
    return out


def fit_sky_dtype(nb_of_bands):
    """The two columns a flux fit with sky adds per galaxy: the fitted background under the galaxy and
    its error."""
    nb = int(nb_of_bands)
    return [("fit_sky", "<f8", (nb,)), ("fit_sky_err", "<f8", (nb,))]


def fit_sky_records(sky_coef, sky_cov, sky_status, places, cutout_size, field_size, field_ptr=None, sky_sigma=None,
                    weighted=False):
    """The recarray of fit_sky_dtype from the per-field arrays of scene_fit_flux_sky - sky_coef (M, bands, q), sky_cov (M,
    bands, q, q), sky_status (M, bands, q) - and the placements (N, 2) of the galaxies (field_ptr (M + 1,) gives every galaxy's
    field; None: one field).  fit_sky is the fitted background sum_t s_t B_t at the stamp's centre pixel (pr + cs // 2, pc +
    cs // 2) of its field, in the basis B_0 = 1, B_1 = (2 r - F + 1) / F, B_2 = (2 c - F + 1) / F; fit_sky_err = sqrt(b^T
    sky_cov b) with b that basis over the fitted terms.  A term with sky_status 5 (dropped) has coefficient exactly 0.0 and no
    variance: it adds nothing to either.  A term with sky_status 4 (a field without a counting pixel) makes both NaN.
    Unweighted, sky_cov is in units of the pixel variance: fit_sky_err is multiplied by sky_sigma ((bands,) or (M, bands)), and
    is NaN without it; weighted=True (the weights carry the noise) takes it as it is, and sky_sigma beside it is a
    ValueError."""
    if weighted and sky_sigma is not None:
        raise ValueError(WEIGHTS_CARRY_THE_NOISE)
    coef = np.asarray(sky_coef, dtype=np.float64)
    if coef.ndim != 3 or coef.shape[2] not in (1, 3):
        raise ValueError(f"expected sky_coef (M, bands, 1 or 3), got {coef.shape}")
    M, nb, q = coef.shape
    cov = np.asarray(sky_cov, dtype=np.float64).reshape(M, nb, q, q)
    status = np.asarray(sky_status, dtype=np.int32).reshape(M, nb, q)
    places = np.asarray(places, dtype=np.int64).reshape(-1, 2)
    n = places.shape[0]
    if field_ptr is None:
        field_ptr = [0, n]
    fp = np.asarray(field_ptr, dtype=np.int64).reshape(-1)
    if fp.shape[0] != M + 1 or fp[0] != 0 or fp[-1] != n or (np.diff(fp) < 0).any():
        raise ValueError(f"field_ptr must have {M + 1} entries, start at 0, never decrease and end at the number of galaxies ({n})")
    sigma = None if sky_sigma is None else check_sky_sigma(sky_sigma, M, nb)
    cs, F = int(cutout_size), int(field_size)
    field = np.repeat(np.arange(M), np.diff(fp))                                  # (N,)
    b = np.ones((n, q))
    if q == 3:
        b[:, 1] = (2 * (places[:, 0] + cs // 2) - F + 1).astype(np.float64) / np.float64(F)
        b[:, 2] = (2 * (places[:, 1] + cs // 2) - F + 1).astype(np.float64) / np.float64(F)
    rec = np.recarray((n,), dtype=fit_sky_dtype(nb))
    with np.errstate(all="ignore"):
        rec["fit_sky"] = np.einsum("nbt,nt->nb", coef[field], b)
        kept = status[field] == 0                                                 # (N, bands, q)
        bk = np.where(kept, b[:, None, :], 0.0)
        var = np.einsum("nbt,nbtu,nbu->nb", bk, np.where(kept[..., :, None] & kept[..., None, :], cov[field], 0.0), bk)
        err = np.where((status[field] == FIT_STATUS_INELIGIBLE).any(axis=2) | ~kept.any(axis=2), np.nan, np.sqrt(var))
        if weighted:
            rec["fit_sky_err"] = err
        elif sigma is None:
            rec["fit_sky_err"] = np.nan
        else:
            rec["fit_sky_err"] = sigma[field] * err
    return rec


def _fit_host_inputs(who, stamps_mean, data_fields, weight_fields, field_ptr, catalogue, sky_sigma, ctx):
    """What fit_fluxes_sky and fit_fluxes_nonneg check and derive before the engine call, every ValueError before any GPU work:
    (stamps float32, data (M, F, F, bands), the checked weight fields or None, field_ptr, the stamp fluxes, the context)"""
    data = np.asarray(data_fields, dtype=np.float64)
    if data.ndim == 3:
        data = data[None]
    M = data.shape[0]
    if weight_fields is not None:
        if sky_sigma is not None:
            raise ValueError(WEIGHTS_CARRY_THE_NOISE)
        weight_fields = E.check_fit_weights(weight_fields, data.shape)
    if data.ndim == 4 and sky_sigma is not None:
        check_sky_sigma(sky_sigma, M, data.shape[-1])
    stamps = np.asarray(stamps_mean, dtype=np.float32)
    if field_ptr is None and M == 1:
        field_ptr = [0, stamps.shape[0]]
    if catalogue is None:
        flux = stamps.sum(axis=(1, 2), dtype=np.float64) if stamps.ndim == 4 else None
    else:
        if "flux" not in catalogue.dtype.names:
            raise ValueError(f"the catalogue lacks the column flux: {who} takes the measure_stamps recarray of the galaxies")
        flux = np.asarray(catalogue["flux"], dtype=np.float64)
    return stamps, data, weight_fields, field_ptr, flux, E.default_context() if ctx is None else ctx


def fit_fluxes_sky(stamps_mean, places, data_fields, sky_order=0, weight_fields=None, field_ptr=None, catalogue=None,
                   sky_sigma=None, min_pivot=1e-8, ctx=None):
    """fit_fluxes (weight_fields None) or fit_fluxes_weighted with a local sky background fitted jointly with the amplitudes
    (DESIGN.md section 7t), as the SDSS deblender, the Tractor and scarlet do: a sky residual under a blend no longer goes into
    the amplitudes of the models with the widest wings.

    parameters: those of fit_fluxes / fit_fluxes_weighted, and
        sky_order: 0, a constant per field and band; 1, a plane s_0 + s_1 B_1 + s_2 B_2 with B_1 = (2 r - F + 1) / F and B_2 =
            (2 c - F + 1) / F of the field pixel (r, c).  The sky is fitted to ALL pixels of the field (weighted: the counting
            ones), not only to those under a stamp
    returns (catalogue, sky): the np.recarray of fit_fluxes (with weight_fields: of fit_fluxes_weighted) plus fit_sky_dtype -
    fit_sky, the fitted background at the centre pixel of the galaxy's stamp, and fit_sky_err (fit_sky_records) - and the
    dictionary of the per-field arrays sky_coef (M, bands, q), sky_cov (M, bands, q, q), sky_status (M, bands, q) and sky_npix
    (M, bands) of Context.scene_fit_flux_sky.  fit_var, and with it fit_scale_err, now carries the covariance with the sky;
    fit_status, fit_gram and fit_proj are those of the fit without sky.  A field without galaxies still gets its sky.
    Unweighted, a non-finite pixel of data_fields ANYWHERE in a field reaches every galaxy of that field through the sky
    sums (without sky it reached only the galaxies whose stamps cover it): mask such pixels with weight_fields.
    """
    q = E.sky_terms(sky_order)                                            # (ValueError before any GPU work)
    stamps, data, weight_fields, field_ptr, flux, ctx = _fit_host_inputs("fit_fluxes_sky", stamps_mean, data_fields, weight_fields,
                                                                         field_ptr, catalogue, sky_sigma, ctx)
    weighted = weight_fields is not None
    out = ctx.scene_fit_flux_sky(stamps, places, data, field_ptr=field_ptr, sky_order=sky_order, weight_fields=weight_fields,
                                 min_pivot=min_pivot)
    if weighted:
        fit = fit_flux_records(*(out[k] for k in E.FIT_FLUX_KEYS), flux, field_ptr=field_ptr, fit_chi2=out["fit_chi2"],
                               fit_npix=out["fit_npix"])
    else:
        fit = fit_flux_records(*(out[k] for k in E.FIT_FLUX_KEYS), flux, sky_sigma=sky_sigma, field_ptr=field_ptr)
    sky = fit_sky_records(out["sky_coef"], out["sky_cov"], out["sky_status"], places, stamps.shape[1], data.shape[1],
                          field_ptr=field_ptr, sky_sigma=sky_sigma, weighted=weighted)
    assert out["sky_coef"].shape[2] == q
    return _join_records(fit, sky), {k: out[k] for k in E.FIT_SKY_KEYS}


def fit_nonneg_dtype(nb_of_bands):
    """The four columns a non-negative flux fit adds per galaxy."""
    nb = int(nb_of_bands)
    return [("fit_scale_free", "<f8", (nb,)), ("flux_fit_free", "<f8", (nb,)), ("fit_clamped", "<i4", (nb,)),
            ("fit_dual", "<f8", (nb,))]


def fit_nonneg_records(fit_scale_free, fit_clamped, fit_dual, flux):
    """The recarray of fit_nonneg_dtype from the three per-galaxy arrays of scene_fit_flux_nonneg, all (N, bands), and the
    stamp fluxes `flux` (N, bands): fit_scale_free, the amplitude of the fit without the constraint (negative where the
    constraint bites); flux_fit_free = fit_scale_free * flux; fit_clamped, 1 where the galaxy was clamped to zero flux;
    fit_dual, the multiplier of a clamped galaxy - how much the residual sum of squares grows per unit of amplitude given
    back to it, halved -, +0.0 of a fitted one, NaN where fit_status is not 0."""
    free = np.asarray(fit_scale_free, dtype=np.float64)
    if free.ndim != 2:
        raise ValueError(f"expected fit_scale_free (N, bands), got {free.shape}")
    n, nb = free.shape
    flux = np.asarray(flux, dtype=np.float64)
    if flux.shape != (n, nb):
        raise ValueError(f"expected flux ({n}, {nb}), got {flux.shape}")
    rec = np.recarray((n,), dtype=fit_nonneg_dtype(nb))
    rec["fit_scale_free"] = free
    rec["fit_clamped"] = np.asarray(fit_clamped, dtype=np.int32).reshape(n, nb)
    rec["fit_dual"] = np.asarray(fit_dual, dtype=np.float64).reshape(n, nb)
    with np.errstate(all="ignore"):
        rec["flux_fit_free"] = free * flux
    return rec


def fit_fluxes_nonneg(stamps_mean, places, data_fields, sky_order=None, weight_fields=None, field_ptr=None, catalogue=None,
                      sky_sigma=None, min_pivot=1e-8, max_iter=100, ctx=None):
    """fit_fluxes, fit_fluxes_weighted or fit_fluxes_sky with the amplitudes constrained to be >= 0, as
    scarlet and the Tractor fit them.  On a noisy field a spurious or very faint detection that overlaps a brighter neighbour
    has about an even chance of a negative amplitude in the linear fit, and its neighbours absorb the light it "gives back";
    clipping afterwards leaves them biased.  Here the same quadratic is minimised subject to a_i >= 0, the sky left free.

    parameters: those of fit_fluxes_sky, and
        sky_order: None fits no sky (the default); 0 or 1 as in fit_fluxes_sky
        max_iter: the cap on the factorisations per field and band, >= 1.  The iteration ends by itself after a handful; a
            field and band that reaches the cap reports nonneg_status 1, and its rows - the last iterate - may be negative
    returns (catalogue, per_field): the np.recarray of the call without the constraint - fit_fluxes, with weight_fields
    fit_fluxes_weighted, with sky_order plus fit_sky_dtype - where fit_scale is exactly 0 for a clamped galaxy and fit_var,
    fit_scale_err, flux_fit_err and fit_independence are NaN there, then fit_nonneg_dtype (fit_nonneg_records); and the
    dictionary of the per-field arrays nonneg_iters and nonneg_status (M, bands) and, with sky_order, those of fit_fluxes_sky.
    A field and band whose unconstrained fit has no negative amplitude has nonneg_iters 1 and the values of the call without
    the constraint, bit for bit.
    """
    if sky_order is not None:
        E.sky_terms(sky_order)                                            # (ValueError before any GPU work)
    E.nonneg_max_iter(max_iter)
    stamps, data, weight_fields, field_ptr, flux, ctx = _fit_host_inputs("fit_fluxes_nonneg", stamps_mean, data_fields,
                                                                         weight_fields, field_ptr, catalogue, sky_sigma, ctx)
    weighted = weight_fields is not None
    out = ctx.scene_fit_flux_nonneg(stamps, places, data, field_ptr=field_ptr, sky_order=sky_order, weight_fields=weight_fields,
                                    min_pivot=min_pivot, max_iter=max_iter)
    if weighted:
        recs = [fit_flux_records(*(out[k] for k in E.FIT_FLUX_KEYS), flux, field_ptr=field_ptr, fit_chi2=out["fit_chi2"],
                                 fit_npix=out["fit_npix"])]
    else:
        recs = [fit_flux_records(*(out[k] for k in E.FIT_FLUX_KEYS), flux, sky_sigma=sky_sigma, field_ptr=field_ptr)]
    per_field = {k: out[k] for k in E.FIT_NONNEG_FIELD_KEYS}
    if sky_order is not None:
        recs.append(fit_sky_records(out["sky_coef"], out["sky_cov"], out["sky_status"], places, stamps.shape[1], data.shape[1],
                                    field_ptr=field_ptr, sky_sigma=sky_sigma, weighted=weighted))
        per_field.update({k: out[k] for k in E.FIT_SKY_KEYS})
    recs.append(fit_nonneg_records(*(out[k] for k in E.FIT_NONNEG_KEYS), flux))
    return _join_records(*recs), per_field


def moments_data_dtype(nb_of_bands):
    """The columns of measure_moments_on_fields' recarray: what the GPU measures on the child image, then
    what the host derives from it."""
    nb = int(nb_of_bands)
    return [("flux_data", "<f8", (nb,)), ("npix_data", "<i4", (nb,)), ("row_data", "<f8"), ("col_data", "<f8"),
            ("Mrr_data", "<f8"), ("Mrc_data", "<f8"), ("Mcc_data", "<f8"), ("iters_data", "<i4"), ("status_data", "<i4"),
            ("sigma_data", "<f8"), ("e1_data", "<f8"), ("e2_data", "<f8"), ("flux_data_err", "<f8", (nb,))]


def moments_data_records(flux_data, npix_data, shape_data, iters_data, status_data, sky_sigma=None, field_ptr=None):
    """The recarray of measure_moments_on_fields from the five arrays the engine returns (scene_moments_fields').  Derived on
    the host: sigma_data, e1_data and e2_data from the moments as catalogue_records derives sigma, e1 and e2 (derived_shape; NaN
    where status_data is 3), and, with sky_sigma (bands,) or (M, bands) - the per-pixel standard deviation of the sky;
    field_ptr (M + 1,) gives every galaxy's field, None: one field - flux_data_err = sky_sigma sqrt(npix_data): the noise of
    the counting pixels, the only ones where the data enter.  Without sky_sigma it is NaN."""
    flux = np.asarray(flux_data, dtype=np.float64)
    if flux.ndim != 2:
        raise ValueError(f"expected flux_data (N, bands), got {flux.shape}")
    n, nb = flux.shape
    npix = np.asarray(npix_data, dtype=np.int32)
    shape = np.asarray(shape_data, dtype=np.float64)
    iters, status = np.asarray(iters_data, dtype=np.int32), np.asarray(status_data, dtype=np.int32)
    if npix.shape != (n, nb) or shape.shape != (n, 5) or iters.shape != (n,) or status.shape != (n,):
        raise ValueError(f"expected npix_data ({n}, {nb}), shape_data ({n}, 5), iters_data and status_data ({n},), got "
                         f"{npix.shape}, {shape.shape}, {iters.shape}, {status.shape}")
    rec = np.recarray((n,), dtype=moments_data_dtype(nb))
    rec["flux_data"], rec["npix_data"] = flux, npix
    for k, name in enumerate(("row_data", "col_data", "Mrr_data", "Mrc_data", "Mcc_data")):
        rec[name] = shape[:, k]
    rec["iters_data"], rec["status_data"] = iters, status
    rec["sigma_data"], rec["e1_data"], rec["e2_data"] = derived_shape(shape, status)
    if sky_sigma is None:
        rec["flux_data_err"] = np.nan
    else:
        if field_ptr is None:
            field_ptr = [0, n]
        fp = np.asarray(field_ptr, dtype=np.int64).reshape(-1)
        M = fp.shape[0] - 1
        if M < 1 or fp[0] != 0 or fp[-1] != n or (np.diff(fp) < 0).any():
            raise ValueError(f"field_ptr must start at 0, never decrease and end at the number of galaxies ({n})")
        sky = check_sky_sigma(sky_sigma, M, nb)[np.repeat(np.arange(M), np.diff(fp))]              # (N, bands)
        rec["flux_data_err"] = sky * np.sqrt(npix.astype(np.float64))
    return rec


def measure_moments_on_fields(stamps_mean, places, data_fields, model_fields, weight_fields=None, field_ptr=None,
                              catalogue=None, sky_sigma=None, band=2, sigma0=3.0, tol=1e-10, max_iter=200, ctx=None):
    """The adaptive moments of measure_stamps re-measured on the observed field with the neighbours' models subtracted, on the
    GPU: per galaxy the child image C = D - T + P, D the observed field, T the composited mean field and
    P the galaxy's own mean stamp, as SExtractor, the SDSS deblender and LSST's deblended children measure shapes.  A network
    that makes a galaxy too round or too large biases the shape of P; it does not bias the shape of C.  Where a stamp pixel lies
    outside the field or under a masked pixel, C is P: the model fills in what is hidden.

    parameters:
        stamps_mean: the network's mean stamps, (N, cutout_size, cutout_size, bands)
        places: (N, 2), the field position (row, col) of every stamp's top-left corner - where the stamp was composited
        data_fields: (M, F, F, bands), the observed fields; (F, F, bands) for one field
        model_fields: the composited mean fields (the sum of all mean stamps of a field), of the same shape
        weight_fields: of the same shape, or None.  A mask only: a pixel counts iff 0 < W < inf, and a NaN or a saturated value
            of the data under a masked pixel reaches nothing.  The moments are not inverse-variance weighted
        field_ptr: (M + 1,), stamps field_ptr[m]:field_ptr[m + 1] lie in field m; None: one field holds them all
        catalogue: the measure_stamps recarray of the same galaxies, or None.  Only its length is checked: the iteration starts
            from the stamp centre and sigma0, as measure_stamps does, not from the model's moments
        sky_sigma: (bands,) or (M, bands), the standard deviation of the sky noise per pixel; None: flux_data_err is NaN
        band, sigma0, tol, max_iter: those of measure_stamps
        ctx: the engine context to run on (None: the default context)
    returns a np.recarray of moments_data_dtype: flux_data (bands,), the sum of C; npix_data (bands,), the counting pixels;
    row_data, col_data, Mrr_data, Mrc_data, Mcc_data, iters_data, status_data, the adaptive moments of band `band` of C with
    measure_stamps' status codes (a non-finite value of D at a counting pixel ends in STATUS_FAILED); and, derived on the host,
    sigma_data, e1_data, e2_data and flux_data_err (moments_data_records).  Where D equals T bit for bit the measured columns
    have the bits of measure_stamps.
    """
    data = np.asarray(data_fields, dtype=np.float64)
    model = np.asarray(model_fields, dtype=np.float64)
    if data.ndim == 3:
        data = data[None]
    if model.ndim == 3:
        model = model[None]
    M = model.shape[0]
    if model.ndim == 4 and sky_sigma is not None:
        check_sky_sigma(sky_sigma, M, model.shape[-1])                   # (ValueError before any GPU work)
    stamps = np.asarray(stamps_mean, dtype=np.float32)
    if catalogue is not None and len(catalogue) != stamps.shape[0]:
        raise ValueError(f"the catalogue has {len(catalogue)} rows for {stamps.shape[0]} stamps: measure_moments_on_fields takes "
                         "the measure_stamps recarray of the same galaxies")
    if field_ptr is None and M == 1:
        field_ptr = [0, stamps.shape[0]]
    if ctx is None:
        ctx = E.default_context()
    out = ctx.scene_moments_fields(stamps, places, model, data, weight_fields=weight_fields, field_ptr=field_ptr, band=band,
                                   sigma0=sigma0, tol=tol, max_iter=max_iter)
    return moments_data_records(out["flux_data"], out["npix_data"], out["shape_data"], out["iters_data"], out["status_data"],
                                sky_sigma=sky_sigma, field_ptr=field_ptr)


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
