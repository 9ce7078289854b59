"""Sub-pixel position fit (reference: src/debvader/deblend_cutout/optimization.py).

The reference fits one galaxy at a time: scipy.optimize.least_squares on
    J(s) = mean over the field of (field[:, :, 2] - shift(shift(pad(mean)[:, :, 2], d), s))^2,  s in [-3, 3]^2,
with scipy.ndimage.shift, a 2-point Jacobian and every objective evaluation shifting a field-sized image.  Here the same
objective is minimised for all galaxies in one engine call (dv_scene_fit_shifts): one GPU workgroup per galaxy, float64,
analytic gradient and Hessian of the B-spline shift, box-projected Newton steps.  Only the r band (index 2) is used, as
in the reference; there is no CPU fallback.
"""
import numpy as np

from debvader_amd import engine as E

R_BAND = 2        # the reference fits on field_image[:, :, 2]


def _field_r(field_image):
    f = np.asarray(field_image)
    if f.ndim == 4 and f.shape[0] == 1:
        f = f[0]
    if f.ndim != 3 or f.shape[0] != f.shape[1]:
        raise ValueError(f"expected a square field (F, F, bands) or (1, F, F, bands), got {np.shape(field_image)}")
    if f.shape[2] <= R_BAND:
        raise ValueError(f"the position fit uses band {R_BAND} (r); this field has {f.shape[2]} band(s)")
    return f[:, :, R_BAND]


def _stamps_r(stamps):
    s = np.asarray(stamps)
    if s.ndim != 4 or s.shape[1] != s.shape[2]:
        raise ValueError(f"expected stamps (N, cs, cs, bands), got {s.shape}")
    if s.shape[3] <= R_BAND:
        raise ValueError(f"the position fit uses band {R_BAND} (r); these stamps have {s.shape[3]} band(s)")
    return s[:, :, :, R_BAND]


def position_optimization_batch(field_image, stamps, distances, bound=3.0, ctx=None, max_iter=50, return_details=False):
    """Fit the sub-pixel shift of every galaxy at once.

    parameters:
        field_image: (F, F, bands) or (1, F, F, bands)
        stamps: (N, cs, cs, bands) predicted images, unpadded (pad() centres them at int((F - cs) / 2))
        distances: (N, 2) distances to the centre as detected, {row, column}
        bound: the box [-bound, bound]^2 of the shifts (3 in the reference)
        ctx: engine context (default: the process's default context)
        return_details: also return the engine's {objective, iters, status} per galaxy
    returns the (N, 2) shifts, {row, column}; with return_details, (shifts, details)
    """
    field_r = _field_r(field_image)
    stamps_r = _stamps_r(stamps)
    dist = np.asarray(distances, dtype=np.float64).reshape(-1, 2)
    if dist.shape[0] != stamps_r.shape[0]:
        raise ValueError(f"{stamps_r.shape[0]} stamps but {dist.shape[0]} distances")
    ctx = ctx or E.default_context()
    r = ctx.scene_fit_shifts(field_r, stamps_r, dist, bound=bound, max_iter=max_iter)
    if return_details:
        return r["shifts"], {k: r[k] for k in ("objective", "iters", "status")}
    return r["shifts"]


def position_optimization_fields(field_images, stamps, distances, field_ptr, bound=3.0, ctx=None, max_iter=50,
                                 return_details=False):
    """position_optimization_batch for the galaxies of many fields in one engine call (dv_scene_fit_shifts_fields).

    parameters:
        field_images: (M, F, F, bands)
        stamps: (N, cs, cs, bands) predicted images of the galaxies of all fields, field after field
        distances: (N, 2) distances to the centre of each galaxy's own field, {row, column}
        field_ptr: (M + 1,) - galaxies field_ptr[m]:field_ptr[m + 1] belong to field m
    returns the (N, 2) shifts; with return_details, (shifts, details).  Every galaxy gets the shift
    position_optimization_batch gives it on its own field, bit for bit.
    """
    f = np.asarray(field_images)
    if f.ndim != 4 or f.shape[1] != f.shape[2]:
        raise ValueError(f"expected square fields (M, F, F, bands), got {f.shape}")
    if f.shape[3] <= R_BAND:
        raise ValueError(f"the position fit uses band {R_BAND} (r); these fields have {f.shape[3]} band(s)")
    stamps_r = _stamps_r(stamps)
    dist = np.asarray(distances, dtype=np.float64).reshape(-1, 2)
    if dist.shape[0] != stamps_r.shape[0]:
        raise ValueError(f"{stamps_r.shape[0]} stamps but {dist.shape[0]} distances")
    fp = E.check_field_ptr(field_ptr, f.shape[0], stamps_r.shape[0])
    ctx = ctx or E.default_context()
    r = ctx.scene_fit_shifts_fields(f[:, :, :, R_BAND], stamps_r, dist, fp, bound=bound, max_iter=max_iter)
    if return_details:
        return r["shifts"], {k: r[k] for k in ("objective", "iters", "status")}
    return r["shifts"]


def position_optimization(field_image, output_image_mean_padded, galaxy_distance_to_center):
    """
    Find shifts in the position of the deblended galaxy to minimize the mse between field_image
    (the reference's name, signature and return; the fit runs on the GPU)

    parameters:
        field image: image of the entire field of galaxy to be deblended, (F, F, bands).
        output_images_mean_padded: predicted image of the galaxy that is to be optimized, padded to (F, F, bands).
        galaxy_distances_to_center: distance of the predicted galaxy from the center, as detected by the detection algorithm.
    returns (shift_x, shift_y)
    """
    padded = np.asarray(output_image_mean_padded)
    if padded.ndim != 3:
        raise ValueError(f"expected a padded image (F, F, bands), got {padded.shape}")
    s = position_optimization_batch(field_image, padded[None], np.asarray(galaxy_distance_to_center, np.float64)[None, :2])
    return s[0, 0], s[0, 1]
