"""Source detection (reference: src/debvader/detect/detection.py).

The reference runs sep (SExtractor's library) on band 2 (r) of the field.  This engine has no sep: the same method -
SExtractor's published algorithm (Bertin & Arnouts 1996) with the rules of DESIGN.md section 7e - runs on the GPU
(Context.scene_detect, csrc/detect.hip), float64, with the reference's settings (thresh 1.5 x globalrms, minarea 4,
64 deblending levels, contrast 1e-5, a 7 x 7 Gaussian matched filter, 64-pixel background meshes).  It is not sep, and
its catalogue is not claimed to equal sep's: INTEGRATION.md lists the known differences.  There is no CPU fallback.
"""
import numpy as np

from debvader_amd import engine as E

R_BAND = 2        # the reference detects on field_image[0, :, :, 2]


def _distances(x, y, field_size):
    """the reference's (row, column) distances to the centre, rounded half to even as np.round does"""
    if len(x) == 0:
        return np.array([])
    h = -int(field_size / 2)
    return np.array([(np.round(h + yy), np.round(h + xx)) for xx, yy in zip(x, y)])


def _bands_r(images):
    a = np.asarray(images)
    if a.ndim != 4:
        raise ValueError(f"expected fields (N, F, F, bands), got {a.shape}")
    if a.shape[3] <= R_BAND:
        raise ValueError(f"detection uses band {R_BAND} (r); these fields have {a.shape[3]} band(s)")
    return a[:, :, :, R_BAND]


def _planes_r(kw, n):
    """the detector's keywords with weights / mask of (N, F, F, bands) cut to band 2, the first n
    fields of them; (N, F, F) planes pass as they are"""
    kw = dict(kw)
    for name in ("weights", "mask"):
        if kw.get(name) is not None:
            a = np.asarray(kw[name])
            kw[name] = _bands_r(a[:n]) if a.ndim == 4 else a[:n]
    return kw


def _multiband(images, ctx, bands, band_weights, kw):
    """Context.scene_detect_multiband on whole fields (N, F, F, bands); weights / mask of
    (N, F, F, bands of the fields) are indexed by `bands`, a three-dimensional mask passes as it is"""
    a = np.asarray(images)
    if a.ndim != 4:
        raise ValueError(f"expected fields (N, F, F, bands), got {a.shape}")
    kw = dict(kw)
    sel = list(range(a.shape[3])) if bands is None else list(bands)
    for name in ("weights", "mask"):
        if kw.get(name) is not None:
            p = np.asarray(kw[name])
            kw[name] = p[:len(a)][:, :, :, sel] if p.ndim == 4 else p[:len(a)]
    ctx = ctx or E.default_context()
    return ctx.scene_detect_multiband(a, bands=bands, band_weights=band_weights, **kw)


_SINGLE = object()      # bands not given: the single-band call on band 2


def detect_objects_batch(field_images, ctx=None, bands=_SINGLE, band_weights=None, **kw):
    """detect_objects for every field of (N, F, F, bands) in one engine call; returns a list of N arrays as
    detect_objects returns them.  kw: the detector's settings (Context.scene_detect), among them weights, mask, noise and
    filter_type: the noise map and the mask that sep takes as err= and mask=.  With bands (a list of band numbers, None for
    all) detection runs on the inverse-variance combination of those bands (Context.scene_detect_multiband, DESIGN.md
    section 7za) with the spectral shape band_weights; four-dimensional weights / mask are then indexed by bands."""
    if bands is not _SINGLE:
        r = _multiband(field_images, ctx, bands, band_weights, kw)
        F, off = np.shape(field_images)[1], r["offsets"]
        return [_distances(r["x"][off[i]:off[i + 1]], r["y"][off[i]:off[i + 1]], F) for i in range(len(off) - 1)]
    if band_weights is not None:
        raise ValueError("band_weights belong to the multi-band call: give bands")
    r_band = _bands_r(field_images)
    kw = _planes_r(kw, len(r_band))
    ctx = ctx or E.default_context()
    r = ctx.scene_detect(r_band, **kw)
    F = r_band.shape[1]
    off = r["offsets"]
    return [_distances(r["x"][off[i]:off[i + 1]], r["y"][off[i]:off[i + 1]], F) for i in range(r_band.shape[0])]


def detect_objects(field_image, ctx=None, bands=_SINGLE, band_weights=None, **kw):
    """
    Detect the objects in the field_image image using the SExtractor detection algorithm (on the GPU).
    field_image: (1, F, F, bands); returns the (row, column) distances of the objects to the centre of the field,
    np.round(-int(F / 2) + barycentre), as an (n, 2) array, or np.array([]) when nothing is found.
    bands, band_weights: as in detect_objects_batch (detection on the combination of several bands).
    """
    field_image = np.asarray(field_image)
    if field_image.ndim != 4 or field_image.shape[0] < 1:
        raise ValueError(f"expected a field (1, F, F, bands), got {field_image.shape}")
    field_size = field_image.shape[1]
    if bands is not _SINGLE:
        r = _multiband(field_image[:1], ctx, bands, band_weights, kw)
        return _distances(r["x"], r["y"], field_size)
    if band_weights is not None:
        raise ValueError("band_weights belong to the multi-band call: give bands")
    r_band = _bands_r(field_image[:1])
    kw = _planes_r(kw, 1)
    ctx = ctx or E.default_context()
    r = ctx.scene_detect(r_band, **kw)
    return _distances(r["x"], r["y"], field_size)
