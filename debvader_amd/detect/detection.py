"""Source detection (reference: src/debvader/detect/detection.py).

The reference runs sep (SExtractor's library) on band 2 (r) of the field.  This engine has no sep: the same method -
SExtractor's published algorithm (Bertin & Arnouts 1996) with the rules of DESIGN.md section 7e - runs on the GPU
(Context.scene_detect, csrc/detect.hip), float64, with the reference's settings (thresh 1.5 x globalrms, minarea 4,
64 deblending levels, contrast 1e-5, a 7 x 7 Gaussian matched filter, 64-pixel background meshes).  It is not sep, and
its catalogue is not claimed to equal sep's: INTEGRATION.md lists the known differences.  There is no CPU fallback.

The reference's sep.extract call leaves sep's defaults clean=True, clean_param=1.0 on: sep drops the objects that would not
have been detected without the wings of a brighter neighbour.  Here that cleaning pass is a mode of
its own, clean=True (clean_param=1.0), off by default so that every existing catalogue keeps its rows.
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


def _pop_clean(kw):
    """(kw without clean / clean_param, clean_param or None): the cleaning pass is asked for with
    clean=True; clean_param (1.0) is checked before anything runs, also when clean is off"""
    kw = dict(kw)
    clean = kw.pop("clean", False)
    clean_param = kw.pop("clean_param", 1.0)
    if not isinstance(clean, (bool, np.bool_)):
        raise ValueError(f"clean must be True or False, got {clean!r}")
    E.check_detect_clean(clean_param, None, None)
    return kw, (float(clean_param) if clean else None)


def _multiband(images, ctx, bands, band_weights, kw, clean_param=None):
    """Context.scene_detect_multiband on whole fields (N, F, F, bands); weights / mask of
    (N, F, F, bands of the fields) are indexed by `bands`, a three-dimensional mask passes as it is.  clean_param: the
    catalogue of Context.scene_detect_clean instead"""
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
    if clean_param is not None:
        return ctx.scene_detect_clean(a, bands=bands, band_weights=band_weights, columns=False, clean_param=clean_param, **kw)
    return ctx.scene_detect_multiband(a, bands=bands, band_weights=band_weights, **kw)


_SINGLE = object()      # bands not given: the single-band call on band 2


def detect_objects_batch(field_images, ctx=None, bands=_SINGLE, band_weights=None, **kw):
    """detect_objects for every field of (N, F, F, bands) in one engine call; returns a list of N arrays as
    detect_objects returns them.  kw: the detector's settings (Context.scene_detect), among them weights, mask, noise and
    filter_type: the noise map and the mask that sep takes as err= and mask=.  With bands (a list of band numbers, None for
    all) detection runs on the inverse-variance combination of those bands (Context.scene_detect_multiband, DESIGN.md
    section 7za) with the spectral shape band_weights; four-dimensional weights / mask are then indexed by bands.
    clean=True (default False), clean_param=1.0: the cleaning pass that the reference's sep call runs with sep's defaults
    (Context.scene_detect_clean): objects that a brighter neighbour's wings explain are merged into it."""
    kw, clean_param = _pop_clean(kw)
    if bands is not _SINGLE:
        r = _multiband(field_images, ctx, bands, band_weights, kw, clean_param)
        F, off = np.shape(field_images)[1], r["offsets"]
        return [_distances(r["x"][off[i]:off[i + 1]], r["y"][off[i]:off[i + 1]], F) for i in range(len(off) - 1)]
    if band_weights is not None:
        raise ValueError("band_weights belong to the multi-band call: give bands")
    r_band = _bands_r(field_images)
    kw = _planes_r(kw, len(r_band))
    ctx = ctx or E.default_context()
    r = ctx.scene_detect(r_band, **kw) if clean_param is None else \
        ctx.scene_detect_clean(r_band, columns=False, clean_param=clean_param, **kw)
    F = r_band.shape[1]
    off = r["offsets"]
    return [_distances(r["x"][off[i]:off[i + 1]], r["y"][off[i]:off[i + 1]], F) for i in range(r_band.shape[0])]


def detect_objects(field_image, ctx=None, bands=_SINGLE, band_weights=None, **kw):
    """
    Detect the objects in the field_image image using the SExtractor detection algorithm (on the GPU).
    field_image: (1, F, F, bands); returns the (row, column) distances of the objects to the centre of the field,
    np.round(-int(F / 2) + barycentre), as an (n, 2) array, or np.array([]) when nothing is found.
    bands, band_weights: as in detect_objects_batch (detection on the combination of several bands).
    clean=True (default False), clean_param=1.0: sep's cleaning pass, which the reference's sep call runs with sep's
    defaults, as in detect_objects_batch.
    """
    kw, clean_param = _pop_clean(kw)
    field_image = np.asarray(field_image)
    if field_image.ndim != 4 or field_image.shape[0] < 1:
        raise ValueError(f"expected a field (1, F, F, bands), got {field_image.shape}")
    field_size = field_image.shape[1]
    if bands is not _SINGLE:
        r = _multiband(field_image[:1], ctx, bands, band_weights, kw, clean_param)
        return _distances(r["x"], r["y"], field_size)
    if band_weights is not None:
        raise ValueError("band_weights belong to the multi-band call: give bands")
    r_band = _bands_r(field_image[:1])
    kw = _planes_r(kw, 1)
    ctx = ctx or E.default_context()
    r = ctx.scene_detect(r_band, **kw) if clean_param is None else \
        ctx.scene_detect_clean(r_band, columns=False, clean_param=clean_param, **kw)
    return _distances(r["x"], r["y"], field_size)


# ---- objects with shapes and a segmentation map -------------------------------------------------
# sep's column names where the meaning is sep's, then this detector's own
_OBJECT_COLUMNS = (("npix", np.int32), ("xmin", np.int32), ("xmax", np.int32), ("ymin", np.int32), ("ymax", np.int32),
                   ("x", np.float64), ("y", np.float64), ("x2", np.float64), ("y2", np.float64), ("xy", np.float64),
                   ("a", np.float64), ("b", np.float64), ("theta", np.float64), ("cxx", np.float64), ("cyy", np.float64),
                   ("cxy", np.float64), ("flux", np.float64), ("peak", np.float64), ("xpeak", np.int32), ("ypeak", np.int32),
                   ("flag", np.int32), ("parent", np.int32), ("dflux", np.float64), ("vpeak", np.float64),
                   ("xvpeak", np.int32), ("yvpeak", np.int32), ("x_iso", np.float64), ("y_iso", np.float64))


def object_dtype():
    """the record type of extract_objects: sep's columns npix .. flag, then parent, dflux, vpeak, xvpeak, yvpeak, x_iso, y_iso"""
    return np.dtype([(name, t) for name, t in _OBJECT_COLUMNS])


def clean_object_dtype():
    """the record type of extract_objects(clean=True): object_dtype(), then nmerged (1 + the objects
    merged into the row) and mthresh"""
    return np.dtype(list(_OBJECT_COLUMNS) + [("nmerged", np.int32), ("mthresh", np.float64)])


def object_records(r, lo=0, hi=None):
    """rows lo:hi of a result of Context.scene_detect_objects (or of FieldSet.detect after set_detect_objects) as a recarray
    of object_dtype(); a, b, theta, cxx, cyy, cxy are derived from x2, y2, xy where the result does not carry them.  A result
    of Context.scene_detect_clean (it carries nmerged) gives clean_object_dtype()"""
    hi = len(r["x"]) if hi is None else hi
    if "a" not in r:
        r = dict(r, **E.detect_object_shapes(r["x2"], r["y2"], r["xy"]))
    dtype = clean_object_dtype() if "nmerged" in r else object_dtype()
    rec = np.recarray(hi - lo, dtype=dtype)
    for name in dtype.names:
        rec[name] = r[name][lo:hi]
    return rec


def extract_objects_batch(field_images, ctx=None, bands=_SINGLE, band_weights=None, segmentation_map=False, **kw):
    """The objects of every field of (N, F, F, bands) with their shapes, as sep.extract gives them: a list of N recarrays of
    object_dtype(), with segmentation_map=True a pair of that list and the maps (N, F, F) int32 (0: no object, k + 1: row k
    of the field's recarray).  Arguments as in detect_objects_batch.  With clean=True (clean_param=1.0) the cleaning pass
    that the reference's sep call runs with sep's defaults follows: the recarrays are the cleaned
    rows of clean_object_dtype() and the maps carry their numbers."""
    kw, clean_param = _pop_clean(kw)
    a = np.asarray(field_images)
    ctx = ctx or E.default_context()
    run = ctx.scene_detect_objects
    if clean_param is not None:
        def run(f, **k):
            return ctx.scene_detect_clean(f, clean_param=clean_param, **k)
    if bands is not _SINGLE:
        if a.ndim != 4:
            raise ValueError(f"expected fields (N, F, F, bands), got {a.shape}")
        kw = dict(kw)
        sel = list(range(a.shape[3])) if bands is None else list(bands)
        for name in ("weights", "mask"):
            if kw.get(name) is not None:
                p = np.asarray(kw[name])
                kw[name] = p[:len(a)][:, :, :, sel] if p.ndim == 4 else p[:len(a)]
        r = run(a, bands=bands, band_weights=band_weights, segmentation_map=segmentation_map, **kw)
    else:
        if band_weights is not None:
            raise ValueError("band_weights belong to the multi-band call: give bands")
        r_band = _bands_r(a)
        r = run(r_band, segmentation_map=segmentation_map, **_planes_r(kw, len(r_band)))
    off = r["offsets"]
    recs = [object_records(r, off[i], off[i + 1]) for i in range(len(off) - 1)]
    return (recs, r["segmap"]) if segmentation_map else recs


def extract_objects(field_image, ctx=None, bands=_SINGLE, band_weights=None, segmentation_map=False, **kw):
    """extract_objects_batch for one field (1, F, F, bands): the recarray, with segmentation_map=True the pair
    (recarray, map (F, F)) that sep.extract(..., segmentation_map=True) returns.  clean=True, clean_param=1.0: sep's
    cleaning pass, which the reference's sep call runs with sep's defaults (as in extract_objects_batch)."""
    field_image = np.asarray(field_image)
    if field_image.ndim != 4 or field_image.shape[0] < 1:
        raise ValueError(f"expected a field (1, F, F, bands), got {field_image.shape}")
    out = extract_objects_batch(field_image[:1], ctx=ctx, bands=bands, band_weights=band_weights,
                                segmentation_map=segmentation_map, **kw)
    return (out[0][0], out[1][0]) if segmentation_map else out[0]
