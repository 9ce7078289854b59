"""Thin numpy-level wrapper over the C-ABI (one Context per process/GPU, one Engine per network).

This is the only module that touches ctypes pointers; the Keras-like objects in debvader_amd.model
sit on top of it.
"""
from __future__ import annotations

import atexit
import collections
import ctypes as C
import os
import sys
import threading
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import DvConfig, check, lib


def make_config(input_shape=(59, 59, 6), latent_dim=32, filters=(32, 64, 128, 256), kernels=(3, 3, 3, 3),
                max_batch=256, **overrides) -> DvConfig:
    cfg = DvConfig()
    check(lib.dv_config_default(C.byref(cfg)))
    if len(filters) != len(kernels):
        raise ValueError("filters and kernels must have the same length")
    if len(filters) > _lib.DV_MAX_LEVELS:
        raise ValueError(f"at most {_lib.DV_MAX_LEVELS} levels")
    cfg.height, cfg.width, cfg.bands = int(input_shape[0]), int(input_shape[1]), int(input_shape[2])
    cfg.latent_dim = int(latent_dim)
    cfg.n_levels = len(filters)
    for i in range(_lib.DV_MAX_LEVELS):
        cfg.filters[i] = int(filters[i]) if i < len(filters) else 0
        cfg.kernels[i] = int(kernels[i]) if i < len(kernels) else 0
    cfg.max_batch = int(max_batch)
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown config field {k}")
        setattr(cfg, k, v)
    return cfg


def arch_specs(cfg: DvConfig) -> List[Tuple[str, Tuple[int, ...], bool]]:
    """(name, shape, trainable) of every tensor in TF-checkpoint order. Host only."""
    n = C.c_int32()
    check(lib.dv_arch_counts(C.byref(cfg), C.byref(n), None, None, None))
    out = []
    for i in range(n.value):
        name = C.create_string_buffer(128)
        shape = (C.c_int64 * 4)()
        nd, tr = C.c_int32(), C.c_int32()
        check(lib.dv_arch_describe(C.byref(cfg), i, name, 128, shape, C.byref(nd), C.byref(tr)))
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(nd.value)), bool(tr.value)))
    return out


def arch_counts(cfg: DvConfig) -> Dict[str, int]:
    n = C.c_int32()
    e, d, t = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib.dv_arch_counts(C.byref(cfg), C.byref(n), C.byref(e), C.byref(d), C.byref(t)))
    return dict(tensors=n.value, encoder=e.value, decoder=d.value, trainable=t.value)


def arch_macs(cfg: DvConfig) -> Tuple[int, int]:
    e, d = C.c_int64(), C.c_int64()
    check(lib.dv_arch_macs(C.byref(cfg), C.byref(e), C.byref(d)))
    return e.value, d.value


def device_count() -> int:
    n = C.c_int32()
    check(lib.dv_device_count(C.byref(n)))
    return n.value


def device_bus_id(device: int) -> str:
    """PCI bus id of visible device `device` ("" when it cannot be had: no GPU, index not visible)."""
    buf = C.create_string_buffer(32)
    if lib.dv_device_bus_id(int(device), buf, 32) != 0:
        return ""
    return buf.value.decode()


def _fp(a: Optional[np.ndarray]):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dp(a: Optional[np.ndarray]):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _i32_rows(a, what: str) -> np.ndarray:
    """Integer (x, y) rows for the C-ABI's int32 arrays.  A plain astype would wrap 64-bit values into range silently -
    a start of 2**32 + 5 would fetch the cutout at 5 - so the range is checked before the cast."""
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        r = np.rint(np.asarray(a, dtype=np.float64))
        if a.size and not np.array_equal(r, np.asarray(a, dtype=np.float64)):
            raise ValueError(f"{what} must be integers")
        a = r
    if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise ValueError(f"{what} outside the int32 range")
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 2)


def check_field_ptr(field_ptr, n_fields: int, n_stamps: int) -> np.ndarray:
    """The field_ptr of the many-field calls (dv_infer_fields*, dv_scene_fit_shifts_fields) as int64 (n_fields + 1,):
    stamps field_ptr[m]:field_ptr[m + 1] belong to field m, so it starts at 0, never decreases and ends at n_stamps."""
    fp = np.asarray(field_ptr)
    if fp.dtype.kind not in "iu":
        r = np.rint(np.asarray(fp, dtype=np.float64))
        if fp.size and not np.array_equal(r, np.asarray(fp, dtype=np.float64)):
            raise ValueError("field_ptr must be integers")
        fp = r
    fp = np.ascontiguousarray(fp, dtype=np.int64)
    if fp.ndim != 1 or fp.shape[0] != int(n_fields) + 1:
        raise ValueError(f"field_ptr must have one entry per field plus one ({int(n_fields) + 1}), got shape {fp.shape}")
    if fp[0] != 0 or fp[-1] != int(n_stamps):
        raise ValueError(f"field_ptr must start at 0 and end at the number of stamps ({int(n_stamps)}), got {fp[0]} .. {fp[-1]}")
    if (np.diff(fp) < 0).any():
        raise ValueError(f"field_ptr must not decrease (it does at field {int(np.argmax(np.diff(fp) < 0))})")
    return fp


def _check_fields(fields) -> np.ndarray:
    fields = np.ascontiguousarray(fields, dtype=np.float64)
    if fields.ndim != 4 or fields.shape[1] != fields.shape[2]:
        raise ValueError(f"expected square fields (M, F, F, bands), got {fields.shape}")
    return fields


def measure_params(band, sigma0, tol, max_iter, bands: int) -> "_lib.DvMeasureParams":
    """The checked dv_measure_params of the measurement calls (the library refuses the same, after the arrays are built)."""
    if int(band) != band or not 0 <= int(band) < int(bands):
        raise ValueError(f"band {band} asked for, the stamps have bands 0 .. {int(bands) - 1}")
    if not (np.isfinite(sigma0) and sigma0 > 0) or not (np.isfinite(tol) and tol > 0):
        raise ValueError(f"sigma0 and tol must be finite and positive (got {sigma0}, {tol})")
    if int(max_iter) != max_iter or int(max_iter) < 0:
        raise ValueError(f"max_iter must be an integer >= 0 (got {max_iter})")
    return _lib.DvMeasureParams(int(band), float(sigma0), float(tol), int(max_iter))


MEASURE_MAX_STAMP = 90      # the float64 band plane of a larger stamp does not fit the measurement kernel's 64 KB of LDS


def check_measure_args(mean, stddev, band, sigma0, tol, max_iter):
    """(mean, stddev, params) of scene_measure: C-contiguous float32 stamps (N, cs, cs, bands), stddev None or of the same
    shape."""
    mean = _f32c(mean)
    if mean.ndim != 4 or mean.shape[1] != mean.shape[2] or mean.shape[1] < 1 or mean.shape[3] < 1:
        raise ValueError(f"expected square stamps (N, cs, cs, bands), got {mean.shape}")
    if mean.shape[1] > MEASURE_MAX_STAMP:
        raise ValueError(f"stamps of {mean.shape[1]} pixels: the measurement takes at most {MEASURE_MAX_STAMP}")
    if stddev is not None:
        stddev = _f32c(stddev)
        if stddev.shape != mean.shape:
            raise ValueError(f"mean stamps {mean.shape} but stddev stamps {stddev.shape}")
    return mean, stddev, measure_params(band, sigma0, tol, max_iter, mean.shape[3])


MC_SHAPE_NAMES = ("row", "col", "Mrr", "Mrc", "Mcc", "sigma", "e1", "e2")     # the columns of shape_mc_mean / shape_mc_std

REGAUSS_MAX_STAMP = 64          # a thread of the correction kernel keeps at most 16 pixels of the corrected plane in registers
REGAUSS_PSF_SIZES = (5, 33)     # PSF images of 5 .. 33 pixels: with a 64-pixel stamp the largest still fits a workgroup's LDS


def check_psf_args(psf, psf_index, n: int, psf_sigma0):
    """(psf, psf_index) of the PSF-corrected measurement: C-contiguous float64 PSF images (K, ps, ps) - one image (ps, ps) is
    K = 1 - and the int32 index (n,) of every galaxy's PSF (None: PSF 0 for all).  An index outside 0 .. K - 1 is not an
    error: that galaxy's row gets regauss_status 5."""
    psf = np.ascontiguousarray(psf, dtype=np.float64)
    if psf.ndim == 2:
        psf = psf[None]
    if psf.ndim != 3 or psf.shape[1] != psf.shape[2] or psf.shape[0] < 1:
        raise ValueError(f"expected square PSF images (K, ps, ps) with K >= 1, got {psf.shape}")
    if not REGAUSS_PSF_SIZES[0] <= psf.shape[1] <= REGAUSS_PSF_SIZES[1]:
        raise ValueError(f"PSF images of {psf.shape[1]} pixels: {REGAUSS_PSF_SIZES[0]} .. {REGAUSS_PSF_SIZES[1]} are taken")
    if not (np.isfinite(psf_sigma0) and psf_sigma0 > 0):
        raise ValueError(f"psf_sigma0 must be finite and positive (got {psf_sigma0})")
    if psf_index is None:
        index = np.zeros(int(n), np.int32)
    else:
        index = np.asarray(psf_index)
        if index.dtype.kind not in "iu":
            raise ValueError("psf_index must be integers")
        if index.shape != (int(n),):
            raise ValueError(f"psf_index must have one entry per galaxy ({int(n)},), got {index.shape}")
        index = np.ascontiguousarray(np.clip(index, -1, 2 ** 31 - 1), dtype=np.int32)     # (any negative index stays out of range)
    return psf, index


def _regauss_out(n, K):
    """The result dictionary of the PSF-corrected measurement and its pointers in the C-ABI's order."""
    out = dict(regauss=np.zeros((n, 6), np.float64), regauss_iters=np.zeros(n, np.int32), regauss_status=np.zeros(n, np.int32),
               psf_shape=np.zeros((K, 5), np.float64), psf_aux=np.zeros((K, 3), np.float64), psf_iters=np.zeros(K, np.int32),
               psf_status=np.zeros(K, np.int32))
    return out, [_dp(out["regauss"]), _ip(out["regauss_iters"]), _ip(out["regauss_status"]), _dp(out["psf_shape"]),
                 _dp(out["psf_aux"]), _ip(out["psf_iters"]), _ip(out["psf_status"])]


APERTURE_MAX_RADII, APERTURE_MAX_FRACTIONS = 8, 4      # what dv_aperture_params holds
APERTURE_KEYS = ("ap_flux", "ap_flux_err", "ap_area", "flux_auto", "flux_auto_err", "kron", "flux_rho", "aper_flags",
                 "aper_status")                        # the outputs of the aperture photometry, in the C-ABI's order


def aperture_params(radii=(3.0, 5.0, 8.0), fractions=(0.2, 0.5, 0.8), subsample=5, kron_factor=2.5, kron_min=3.5,
                    kron_limit=6.0, bisect_iters=32) -> "_lib.DvApertureParams":
    """The checked dv_aperture_params of the aperture photometry (the library refuses the same, after the arrays are
    built): up to 8 radii in pixels, up to 4 flux fractions strictly between 0 and 1."""
    radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    fractions = np.asarray(fractions, dtype=np.float64).reshape(-1)
    if radii.size > APERTURE_MAX_RADII or fractions.size > APERTURE_MAX_FRACTIONS:
        raise ValueError(f"{radii.size} aperture radii and {fractions.size} flux fractions: at most {APERTURE_MAX_RADII} "
                         f"radii and {APERTURE_MAX_FRACTIONS} fractions are taken")
    if not np.all(np.isfinite(radii) & (radii > 0)):
        raise ValueError(f"aperture radii must be finite and positive (got {radii.tolist()})")
    if not np.all((fractions > 0) & (fractions < 1)):
        raise ValueError(f"flux fractions must lie strictly between 0 and 1 (got {fractions.tolist()})")
    if int(subsample) != subsample or not 1 <= int(subsample) <= 9:
        raise ValueError(f"subsample must be an integer 1 .. 9 (got {subsample})")
    if int(bisect_iters) != bisect_iters or not 1 <= int(bisect_iters) <= 60:
        raise ValueError(f"bisect_iters must be an integer 1 .. 60 (got {bisect_iters})")
    for name, v in (("kron_factor", kron_factor), ("kron_min", kron_min), ("kron_limit", kron_limit)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name} must be finite and positive (got {v})")
    par = _lib.DvApertureParams()
    par.n_radii, par.n_fractions, par.subsample, par.bisect_iters = radii.size, fractions.size, int(subsample), int(bisect_iters)
    for k, v in enumerate(radii):
        par.radii[k] = float(v)
    for k, v in enumerate(fractions):
        par.fractions[k] = float(v)
    par.kron_factor, par.kron_min, par.kron_limit = float(kron_factor), float(kron_min), float(kron_limit)
    return par


def _aperture_out(n, nb, par, err=True):
    """The result dictionary of the aperture photometry and its pointers in the C-ABI's order (the two errors only with a
    stddev stamp; an output without rows - no radii, no fractions - goes as a null pointer)."""
    K, J = par.n_radii, par.n_fractions
    out = dict(ap_flux=np.zeros((n, K, nb), np.float64), ap_flux_err=np.zeros((n, K, nb), np.float64),
               ap_area=np.zeros((n, K), np.float64), flux_auto=np.zeros((n, nb), np.float64),
               flux_auto_err=np.zeros((n, nb), np.float64), kron=np.zeros((n, 3), np.float64),
               flux_rho=np.zeros((n, J), np.float64), aper_flags=np.zeros(n, np.int32), aper_status=np.zeros(n, np.int32))
    if not err:
        del out["ap_flux_err"], out["flux_auto_err"]
    ptrs = []
    for k in APERTURE_KEYS:
        a = out.get(k)
        empty = a is None or (K == 0 and k.startswith("ap_")) or (J == 0 and k == "flux_rho")
        ptrs.append(None if empty else (_ip(a) if a.dtype == np.int32 else _dp(a)))
    return out, ptrs


APERTURE_FIELD_KEYS = ("ap_model_sum", "ap_data_sum", "ap_field_area", "auto_model_sum", "auto_data_sum", "auto_field_area")


def _aperture_field_out(n, nb, par):
    """The result dictionary of the apertures on the fields and its pointers in the C-ABI's order (an output without rows -
    no radii - goes as a null pointer)."""
    K = par.n_radii
    out = dict(ap_model_sum=np.zeros((n, K, nb), np.float64), ap_data_sum=np.zeros((n, K, nb), np.float64),
               ap_field_area=np.zeros((n, K), np.float64), auto_model_sum=np.zeros((n, nb), np.float64),
               auto_data_sum=np.zeros((n, nb), np.float64), auto_field_area=np.zeros(n, np.float64))
    return out, [None if K == 0 and k.startswith("ap_") else _dp(out[k]) for k in APERTURE_FIELD_KEYS]


FIT_FLUX_KEYS = ("fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status")
FIT_FLUX_WEIGHTED_KEYS = FIT_FLUX_KEYS + ("fit_chi2", "fit_npix")      # the weighted fit
FIT_FLUX_MAX_N = 1024       # galaxies per field of the dense flux fit (DV_FIT_MAX_N)


def fit_flux_params(min_pivot=1e-8, scratch_bytes=256 << 20) -> "_lib.DvFitFluxParams":
    """The checked dv_fit_flux_params of the flux-fit calls (the library refuses the same)."""
    if not (np.isfinite(min_pivot) and 0.0 < min_pivot < 1.0):
        raise ValueError(f"min_pivot must lie strictly between 0 and 1 (got {min_pivot})")
    if int(scratch_bytes) != scratch_bytes or int(scratch_bytes) < 1:
        raise ValueError(f"scratch_bytes must be an integer >= 1 (got {scratch_bytes})")
    return _lib.DvFitFluxParams(float(min_pivot), int(scratch_bytes))


def _fit_flux_out(n, nb, weighted=False):
    """The result dictionary of the flux fit and its pointers in the C-ABI's order (weighted: with fit_chi2 and fit_npix)."""
    out = {k: np.zeros((n, nb), np.float64) for k in FIT_FLUX_KEYS[:4]}
    out["fit_status"] = np.zeros((n, nb), np.int32)
    ptrs = [_dp(out[k]) for k in FIT_FLUX_KEYS[:4]] + [_ip(out["fit_status"])]
    if weighted:
        out["fit_chi2"], out["fit_npix"] = np.zeros((n, nb), np.float64), np.zeros((n, nb), np.int32)
        ptrs += [_dp(out["fit_chi2"]), _ip(out["fit_npix"])]
    return out, ptrs


FIT_SKY_KEYS = ("sky_coef", "sky_cov", "sky_status", "sky_npix")       # per field: the sky fitted jointly


def sky_terms(sky_order) -> int:
    """The sky terms per field and band of a flux fit with sky: order 0, a constant, 1; order 1, a plane, 3"""
    if isinstance(sky_order, bool) or sky_order not in (0, 1):
        raise ValueError(f"sky_order must be 0 (a constant) or 1 (a plane), got {sky_order!r}")
    return 1 if sky_order == 0 else 3


def _fit_sky_out(M, nb, q):
    """The per-field arrays of a flux fit with sky and their pointers in the C-ABI's order"""
    out = dict(sky_coef=np.zeros((M, nb, q), np.float64), sky_cov=np.zeros((M, nb, q, q), np.float64),
               sky_status=np.zeros((M, nb, q), np.int32), sky_npix=np.zeros((M, nb), np.int64))
    return out, [_dp(out["sky_coef"]), _dp(out["sky_cov"]), _ip(out["sky_status"]),
                 out["sky_npix"].ctypes.data_as(C.POINTER(C.c_int64))]


FIT_NONNEG_KEYS = ("fit_scale_free", "fit_clamped", "fit_dual")       # per galaxy: the non-negative fit
FIT_NONNEG_FIELD_KEYS = ("nonneg_iters", "nonneg_status")             # per field and band


def nonneg_max_iter(max_iter) -> int:
    """The checked iteration cap of a non-negative flux fit (the library refuses the same)"""
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"max_iter must be an integer >= 1 (got {max_iter!r})")
    return int(max_iter)


def _fit_nonneg_out(n, M, nb):
    """The arrays a non-negative flux fit adds - three per galaxy, two per field - and their pointers in the C-ABI's order"""
    out = dict(fit_scale_free=np.zeros((n, nb), np.float64), fit_clamped=np.zeros((n, nb), np.int32),
               fit_dual=np.zeros((n, nb), np.float64), nonneg_iters=np.zeros((M, nb), np.int32),
               nonneg_status=np.zeros((M, nb), np.int32))
    return out, [_dp(out["fit_scale_free"]), _ip(out["fit_clamped"]), _dp(out["fit_dual"]), _ip(out["nonneg_iters"]),
                 _ip(out["nonneg_status"])]


def _fit_sky_args(sky_order, M, nb):
    """A non-negative call's sky: (arrays, order for the C ABI, pointers) - sky_order None is no sky: order -1, NULL outputs"""
    if sky_order is None:
        return {}, -1, [None, None, None, None]
    sky, ptrs = _fit_sky_out(M, nb, sky_terms(sky_order))
    return sky, int(sky_order), ptrs


def _fit_scene_inputs(stamps, places, data_fields, field_ptr):
    """The checked host arrays of scene_fit_flux_sky and scene_fit_flux_nonneg: (stamps float32 (N, cs, cs, bands), places int32
    (N, 2), data float64 (M, F, F, bands), field_ptr int64 (M + 1,)); field_ptr None: one field holds every stamp"""
    stamps = np.ascontiguousarray(stamps, dtype=np.float32)
    if stamps.ndim != 4 or stamps.shape[1] != stamps.shape[2]:
        raise ValueError(f"expected square stamps (N, cs, cs, bands), got {stamps.shape}")
    n, nb = stamps.shape[0], stamps.shape[3]
    data = np.ascontiguousarray(data_fields, dtype=np.float64)
    if data.ndim != 4 or data.shape[1] != data.shape[2] or data.shape[3] != nb:
        raise ValueError(f"expected data fields (M, F, F, {nb}), got {data.shape}")
    places = _i32_rows(places, "stamp placements") if n else np.zeros((0, 2), np.int32)
    if places.shape != (n, 2):
        raise ValueError(f"expected places ({n}, 2), got {places.shape}")
    M = data.shape[0]
    if field_ptr is None:
        if M != 1:
            raise ValueError(f"field_ptr is needed with {M} fields")
        field_ptr = [0, n]
    return stamps, places, data, check_field_ptr(field_ptr, M, n)


def check_fit_weights(weight_fields, shape):
    """The C-contiguous float64 weight fields of a weighted flux fit: they have the shape of the data fields (M, F, F, bands);
    a 3-d array is taken as one field.  The values are not looked at - the kernel's comparison 0 < W < inf is the rule."""
    w = np.asarray(weight_fields)
    if w.ndim == 3:
        w = w[None]
    if w.shape != tuple(shape):
        raise ValueError(f"expected weight fields of the shape of the data fields {tuple(shape)}, got {np.shape(weight_fields)}")
    return np.ascontiguousarray(w, dtype=np.float64)


def _moments_data_out(n, nb):
    """The result dictionary of the moments on the child images and its pointers in the C-ABI's order."""
    out = dict(flux_data=np.zeros((n, nb), np.float64), npix_data=np.zeros((n, nb), np.int32),
               shape_data=np.zeros((n, 5), np.float64), iters_data=np.zeros(n, np.int32), status_data=np.zeros(n, np.int32))
    return out, [_dp(out["flux_data"]), _ip(out["npix_data"]), _dp(out["shape_data"]), _ip(out["iters_data"]),
                 _ip(out["status_data"])]


def check_measure_mc_args(samples, band, sigma0, tol, max_iter):
    """(samples, params) of scene_measure_mc: C-contiguous float32 sample stamps (S, N, cs, cs, bands), S >= 1."""
    samples = _f32c(samples)
    if samples.ndim != 5 or samples.shape[2] != samples.shape[3] or samples.shape[2] < 1 or samples.shape[4] < 1:
        raise ValueError(f"expected sample stamps (S, N, cs, cs, bands), got {samples.shape}")
    if samples.shape[0] < 1:
        raise ValueError("at least one Monte-Carlo sample per galaxy is needed, got 0")
    if samples.shape[2] > MEASURE_MAX_STAMP:
        raise ValueError(f"stamps of {samples.shape[2]} pixels: the measurement takes at most {MEASURE_MAX_STAMP}")
    return samples, measure_params(band, sigma0, tol, max_iter, samples.shape[4])


def _measure_mc_out(n, nb, S, keep_samples):
    """The result dictionary of the Monte-Carlo catalogue calls and its pointers in the C-ABI's order."""
    out = dict(flux_mc_mean=np.zeros((n, nb), np.float64), flux_mc_std=np.zeros((n, nb), np.float64),
               shape_mc_mean=np.zeros((n, 8), np.float64), shape_mc_std=np.zeros((n, 8), np.float64),
               n_ok=np.zeros(n, np.int32))
    if keep_samples:
        out.update(sample_flux=np.zeros((n, S, nb), np.float64), sample_shape=np.zeros((n, S, 5), np.float64),
                   sample_status=np.zeros((n, S), np.int32))
    ptrs = [_dp(out["flux_mc_mean"]), _dp(out["flux_mc_std"]), _dp(out["shape_mc_mean"]), _dp(out["shape_mc_std"]),
            _ip(out["n_ok"]), _dp(out.get("sample_flux")), _dp(out.get("sample_shape")),
            _ip(out["sample_status"]) if keep_samples else None]
    return out, ptrs


def check_detect_args(fields_r, thresh, minarea, nthresh, cont, filter_kernel, back_size, back_filter,
                      workspace_bytes=0, weights=None) -> np.ndarray:
    """Context.scene_detect's argument checks (before any GPU work); returns the fields as float64 (M, H, W).  weights
    (M, H, W): the weighted call, where the fields must be finite only at the counting pixels."""
    f = np.ascontiguousarray(fields_r, dtype=np.float64)
    if f.ndim != 3 or f.shape[1] < 1 or f.shape[2] < 1:
        raise ValueError(f"expected fields (M, H, W), got {f.shape}")
    if not np.isfinite(f).all():                      # (one pass over the fields; the weights are read only behind a miss)
        if weights is None:
            raise ValueError("the fields must be finite")
        if not np.isfinite(f[counting_pixels(weights)]).all():
            raise ValueError("the fields must be finite at every pixel that counts (0 < weight < inf)")
    if not (np.isfinite(thresh) and np.isfinite(cont)) or int(minarea) < 1 or not 1 <= int(nthresh) <= 1024:
        raise ValueError(f"thresh and cont must be finite, minarea >= 1 and nthresh 1 .. 1024 "
                         f"(got {thresh}, {cont}, {minarea}, {nthresh})")
    if not 1 <= int(back_size) <= 64 or int(back_filter) not in (1, 3, 5, 7) or int(workspace_bytes) < 0:
        raise ValueError(f"back_size must be 1 .. 64 and back_filter odd 1 .. 7 (got {back_size}, {back_filter})")
    if filter_kernel is not None:
        k = np.asarray(filter_kernel, dtype=np.float64)
        if k.ndim != 2 or k.shape[0] % 2 == 0 or k.shape[1] % 2 == 0 or max(k.shape) > 15 \
                or not np.isfinite(k).all() or not np.abs(k).sum() > 0:
            raise ValueError(f"filter_kernel must be a finite, non-zero, odd-sized 2-d array up to 15 x 15, got shape "
                             f"{k.shape}")
    return f


def check_detect_weights(shape, weights, mask, noise, filter_type, thresh):
    """The weight arguments of Context.scene_detect and FieldSet.set_detect_weights, checked before
    any GPU work, for fields of `shape` (M, H, W).  weights: inverse variances or relative weights, a pixel counts iff
    0 < w < inf; mask: booleans, True = bad, zeroes the weights; mask alone: unit weights and noise "relative"; noise
    defaults to "absolute" when weights are given.  Returns (planes float64 (M, H, W), DV_DETECT_NOISE_*, DV_DETECT_FILTER_*)."""
    shape = tuple(int(n) for n in shape)
    if weights is None and mask is None:
        raise ValueError("weighted detection needs weights, a mask or both")
    if noise is None:
        noise = "absolute" if weights is not None else "relative"
    if noise not in _lib.DETECT_NOISE:
        raise ValueError(f"noise must be 'absolute' (the weights are inverse variances, thresh in sigma) or 'relative' "
                         f"(relative weights, thresh in units of globalrms), got {noise!r}")
    if filter_type not in _lib.DETECT_FILTER:
        raise ValueError(f"filter_type must be 'conv' or 'matched', got {filter_type!r}")
    if weights is None:
        w = np.ones(shape, np.float64)
    else:
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if mask is not None:
            w = w.copy()                                  # (the caller's array is kept)
        if w.shape != shape:
            raise ValueError(f"expected weights of the fields' shape {shape}, got {w.shape}")
    if mask is not None:
        m = np.asarray(mask)
        if m.dtype != np.bool_ or m.shape != shape:
            raise ValueError(f"expected a boolean mask (True = bad) of the fields' shape {shape}, got {m.dtype} {m.shape}")
        w[m] = 0.0
    if noise == "absolute" and not float(thresh) > 0:
        raise ValueError(f"with noise='absolute' thresh is in units of the pixel's sigma and must be > 0, got {thresh}")
    return w, _lib.DETECT_NOISE[noise], _lib.DETECT_FILTER[filter_type]


def check_detect_bands(nb, bands, band_weights):
    """The band selection of Context.scene_detect_multiband and FieldSet.set_detect_bands for fields
    of nb bands, checked before any GPU work: k distinct band numbers (None: all), 1 <= k <= nb, and finite band_weights
    c_j > 0 (None: all 1.0).  Returns (bands int32 (k,), band_weights float64 (k,))."""
    nb = int(nb)
    b = np.arange(nb) if bands is None else np.asarray(list(np.atleast_1d(bands)))
    if b.ndim != 1 or not 1 <= len(b) <= nb or not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"bands must be 1 .. {nb} distinct band numbers, got {bands!r}")
    if (b < 0).any() or (b >= nb).any() or len(np.unique(b)) != len(b):
        raise ValueError(f"bands must be distinct and within the fields' {nb} band(s), got {b.tolist()}")
    c = np.ones(len(b), np.float64) if band_weights is None else np.ascontiguousarray(band_weights, dtype=np.float64)
    if c.shape != b.shape or not (np.isfinite(c) & (c > 0)).all():
        raise ValueError(f"band_weights must be {len(b)} finite values > 0, got {band_weights!r}")
    return np.ascontiguousarray(b, dtype=np.int32), c


def check_detect_band_planes(shape, weights, mask, noise, filter_type, thresh):
    """The planes of the multi-band detector for fields (M, H, W) and k selected bands, shape = (M, H, W, k): weights
    (M, H, W, k) as in check_detect_weights; mask (M, H, W) or (M, H, W, k), True = bad, zeroes the planes; a mask alone means
    unit planes and noise "relative".  thresh must be > 0 whatever the noise: it is in units of the combined pixel's sigma.
    Returns (planes float64 (M, H, W, k) or None, DV_DETECT_NOISE_*, DV_DETECT_FILTER_*)."""
    shape = tuple(int(n) for n in shape)
    if filter_type not in _lib.DETECT_FILTER:
        raise ValueError(f"filter_type must be 'conv' or 'matched', got {filter_type!r}")
    if not float(thresh) > 0:
        raise ValueError(f"multi-band detection: thresh is in units of the combined pixel's sigma and must be > 0, got {thresh}")
    if weights is None and mask is None:
        if noise is not None:
            raise ValueError("noise belongs to the planes: give weights, a mask or both")
        return None, 0, _lib.DETECT_FILTER[filter_type]
    if mask is not None:
        m = np.asarray(mask)
        if m.dtype != np.bool_ or m.shape not in (shape, shape[:3]):
            raise ValueError(f"expected a boolean mask (True = bad) of shape {shape[:3]} or {shape}, got {m.dtype} {m.shape}")
        mask = np.ascontiguousarray(np.broadcast_to(m if m.ndim == 4 else m[..., None], shape))
    return check_detect_weights(shape, weights, mask, noise, filter_type, thresh)


def check_detect_clean(clean_param, thresh, minarea):
    """The arguments of the cleaning pass (Context.scene_detect_clean, FieldSet.set_detect_clean),
    checked before any GPU work: clean_param finite and > 0, thresh > 0, minarea <= 64."""
    try:
        ok = np.isfinite(float(clean_param)) and float(clean_param) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok or isinstance(clean_param, (bool, np.bool_)):
        raise ValueError(f"clean_param must be a finite number > 0, got {clean_param!r}")
    if thresh is not None and not float(thresh) > 0:
        raise ValueError(f"the cleaning pass compares profiles with the threshold: thresh must be > 0, got {thresh}")
    if minarea is not None and int(minarea) > _lib.DETECT_CLEAN_MINAREA_MAX:
        raise ValueError(f"the cleaning pass takes minarea up to {_lib.DETECT_CLEAN_MINAREA_MAX}, got {minarea}")


OBJECT_KEYS = _lib.DETECT_OBJECT_INT + _lib.DETECT_OBJECT_DOUBLE
CLEAN_KEYS = ("nmerged", "mthresh")
OBJECT_DERIVED = ("a", "b", "theta", "cxx", "cyy", "cxy")


def detect_object_shapes(x2, y2, xy) -> Dict[str, np.ndarray]:
    """The ellipse of the isophotal moments, derived on the host as sigma, e1 and e2 are for the
    catalogue: a, b the semi-axes, theta the position angle of a from the x axis (0 where both arguments of atan2 are 0),
    and SExtractor's cxx, cyy, cxy."""
    x2, y2, xy = (np.asarray(v, dtype=np.float64) for v in (x2, y2, xy))
    p, d = x2 + y2, x2 - y2
    t = np.sqrt(d * d / 4.0 + xy * xy)
    det = x2 * y2 - xy * xy
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(a=np.sqrt(p / 2.0 + t), b=np.sqrt(np.maximum(p / 2.0 - t, 0.0)),
                   theta=np.where((xy == 0.0) & (d == 0.0), 0.0, 0.5 * np.arctan2(2.0 * xy, d)),
                   cxx=y2 / det, cyy=x2 / det, cxy=-2.0 * xy / det)
    return out


def _object_buffers(cap, segmap_shape=None, columns=True):
    """(arrays, dv_detect_objects) for cap rows: the columns (when asked for) and the segmap (when a shape is given)"""
    arr = {}
    if columns:
        arr.update({k: np.zeros(cap, np.int32) for k in _lib.DETECT_OBJECT_INT})
        arr.update({k: np.zeros(cap, np.float64) for k in _lib.DETECT_OBJECT_DOUBLE})
    if segmap_shape is not None:
        arr["segmap"] = np.zeros(segmap_shape, np.int32)
    st = _lib.DvDetectObjects(**{k: (_ip(v) if v.dtype == np.int32 else _dp(v)) for k, v in arr.items()})
    return arr, st


CATALOG_KEYS = ("field", "parent", "npix", "peak", "flux", "x", "y")


def _detect_params(thresh, cont, minarea, nthresh, back_size, back_filter, filter_kernel, workspace_bytes):
    """(dv_detect_params, the kernel array it points into: the caller keeps it alive for the call)"""
    kern, kptr, kh, kw = None, None, 0, 0
    if filter_kernel is not None:
        kern = np.ascontiguousarray(filter_kernel, dtype=np.float64)
        kptr, (kh, kw) = _dp(kern), kern.shape
    params = _lib.DvDetectParams(float(thresh), float(cont), int(minarea), int(nthresh), int(back_size), int(back_filter),
                                 kptr, kh, kw, int(workspace_bytes))
    return params, kern


def _check_multiband_finite(f, sel, planes):
    """fields (M, H, W, nb) of the multi-band detector: finite in the selected bands, with planes only where the band counts"""
    if np.isfinite(f).all():                          # (one pass over the fields; bands are selected only behind a miss)
        return
    fsel = f[:, :, :, sel]
    if planes is None and not np.isfinite(fsel).all():
        raise ValueError("the fields must be finite in the selected bands")
    if planes is not None and not np.isfinite(fsel[counting_pixels(planes)]).all():
        raise ValueError("the fields must be finite in every selected band where that band counts (0 < weight < inf)")


def _run_detect(M, field_pixels, call):
    """The catalogue of a detect call for M fields of field_pixels pixels each, whose size is known only after the call:
    call(cap, n, offsets, globalrms, columns) makes the library call with room for cap rows - the arguments are the pointers
    in the C ABI's order, columns the seven of CATALOG_KEYS - and is made once unless the catalogue exceeds one object per
    1024 pixels, then once more at the exact size.  Returns ({the columns trimmed to their rows (copies), offsets (M + 1,),
    globalrms (M,)}, rows)."""
    offsets = np.zeros(M + 1, np.int64)
    grms = np.zeros(M, np.float64)
    cap = max(4096, 64 * M, M * field_pixels // 1024)
    while True:
        cat = {k: np.empty(cap, np.int32 if k in ("field", "parent", "npix") else np.float64) for k in CATALOG_KEYS}
        n = C.c_int64()
        call(cap, C.byref(n), offsets.ctypes.data_as(C.POINTER(C.c_int64)), _dp(grms),
             [_ip(cat[k]) if cat[k].dtype == np.int32 else _dp(cat[k]) for k in CATALOG_KEYS])
        if n.value <= cap:
            break
        cap = n.value
    out = {k: v[:n.value].copy() for k, v in cat.items()}
    out.update(offsets=offsets, globalrms=grms)
    return out, n.value


def counting_pixels(w):
    """the pixels that count: 0 < w < inf (NaN does not)"""
    with np.errstate(invalid="ignore"):
        return (w > 0) & (w < np.inf)


def _scene_detect_objects(ctx, fields, bands, band_weights, thresh, minarea, nthresh, cont, filter_kernel, back_size,
                          back_filter, workspace_bytes, weights, mask, noise, filter_type, segmentation_map, columns,
                          clean_param) -> Dict[str, np.ndarray]:
    """Context.scene_detect_objects (clean_param None) and Context.scene_detect_clean: the checks, all before the context is
    touched, the buffers and the library call"""
    clean = clean_param is not None
    if not float(thresh) >= 0:
        raise ValueError(f"the object shapes weight every pixel with D > thresh: thresh must be >= 0, got {thresh}")
    if not (columns or segmentation_map or clean):
        raise ValueError("nothing asked for: columns, segmentation_map or both")
    f = np.ascontiguousarray(fields, dtype=np.float64)
    multi = f.ndim == 4
    bstruct, wstruct, bgrms = None, None, None
    if multi:
        if min(f.shape[1:]) < 1:
            raise ValueError(f"expected fields (M, H, W, bands), got {f.shape}")
        M, H, W, nb = f.shape
        sel, cw = check_detect_bands(nb, bands, band_weights)
        planes, noise_id, filter_id = check_detect_band_planes((M, H, W, len(sel)), weights, mask, noise, filter_type, thresh)
        _check_multiband_finite(f, sel, planes)
        check_detect_args(np.zeros((0, H, W)), thresh, minarea, nthresh, cont, filter_kernel, back_size, back_filter,
                          workspace_bytes)
        bstruct = _lib.DvDetectBands(_ip(sel), len(sel), _dp(cw), _dp(planes), noise_id, filter_id)
    else:
        if bands is not None or band_weights is not None:
            raise ValueError("bands and band_weights belong to fields (M, H, W, bands)")
        nb = 0
        wts = None
        if weights is not None or mask is not None:
            shape = np.shape(fields)
            if len(shape) != 3:
                raise ValueError(f"expected fields (M, H, W) or (M, H, W, bands), got {shape}")
            wts, noise_id, filter_id = check_detect_weights(shape, weights, mask, noise, filter_type, thresh)
            wstruct = _lib.DvDetectWeights(_dp(wts), noise_id, filter_id)
        elif noise is not None or filter_type != "conv":
            raise ValueError("noise and filter_type belong to the weighted call: give weights, a mask or both")
        f = check_detect_args(f, thresh, minarea, nthresh, cont, filter_kernel, back_size, back_filter, workspace_bytes,
                              weights=wts)
        M, H, W = f.shape
    params, kern = _detect_params(thresh, cont, minarea, nthresh, back_size, back_filter, filter_kernel, workspace_bytes)
    obj = {}
    n_raw = np.zeros(M, np.int64)

    def call(cap, n, offsets, grms, catalogue):       # (the object buffers of this size: a retry makes its own)
        arrays, ostruct = _object_buffers(cap, (M, H, W) if segmentation_map else None, columns)
        obj.clear()
        obj.update(arrays)
        args = [ctx._h, _dp(f), M, H, W, nb, C.byref(params), cap, n, offsets, grms, *catalogue,
                None if wstruct is None else C.byref(wstruct), None if bstruct is None else C.byref(bstruct)]
        if not clean:
            check(lib.dv_scene_detect_objects(*args, C.byref(ostruct)))
            return
        obj.update(nmerged=np.zeros(cap, np.int32), mthresh=np.zeros(cap, np.float64))
        cstruct = _lib.DvDetectClean(clean_param, _ip(obj["nmerged"]), _dp(obj["mthresh"]),
                                     n_raw.ctypes.data_as(C.POINTER(C.c_int64)))
        check(lib.dv_scene_detect_clean(*args, C.byref(ostruct) if (columns or segmentation_map) else None,
                                        C.byref(cstruct)))

    out, rows = _run_detect(M, H * W, call)
    out.update({key: (v if key == "segmap" else v[:rows].copy()) for key, v in obj.items()})
    if clean:
        out["n_raw"] = n_raw
    if columns:
        out.update(detect_object_shapes(out["x2"], out["y2"], out["xy"]))
    return out


class _Lease:
    """Owner token of one hand-out of a pool block.  The array the caller receives is built on this object
    (__array_interface__), so numpy makes it the END of the `base` chain of that array and of everything derived from it -
    views, reshapes, the object columns of a recarray, a memoryview, np.frombuffer of one.  When the last of them dies the
    token dies, and its weakref.finalize puts the block back on the pool's return queue."""

    __slots__ = ("_mem", "__array_interface__", "__weakref__")

    def __init__(self, mem: np.ndarray, nbytes: int):
        self._mem = mem                                     # keeps the block alive while the lease is
        self.__array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (mem.ctypes.data, False), "version": 3}


class _HostPool:
    """Recycles the host memory of large result arrays across calls.

    DeblendField.deblend_field returns 16 bytes per pixel and band and galaxy (float64 cutout, float32 mean and stddev): 11 GB
    per 32 768 galaxies.  Fresh np.empty arrays cost a page fault per 4 KiB while the engine's copy threads fill them and
    an munmap of the same size when the previous result is dropped - together more than the GPU work of the call
    (tools/probes/df_lines.py: 0.21 s engine call, 0.25 - 0.5 s freeing the previous recarray).

    Ownership (round 6; until then the pool looked at sys.getrefcount of its blocks, without a lock).  A hand-out is an
    array whose `base` chain ends in a _Lease token that only that array and its descendants reference; the pool itself
    keeps no reference to the token, only a weakref.finalize on it.  A block goes back to the idle list when - and only when -
    its token has been collected, i.e. when no array, view, recarray column, memoryview or np.frombuffer of the hand-out
    is alive.  What Python cannot see it cannot protect: a RAW ADDRESS taken from a result (arr.ctypes.data, a pointer kept
    by a C extension) does not keep the token alive - whoever holds one must keep the array too, or copy.
    Thread safety: empty() runs under a lock from the scan to the finished view; finalizers (which may run on any thread,
    also inside empty() through the garbage collector) only append to a deque, which empty() drains under the lock.
    Bounds: the pool never tracks more than `cap` bytes (leased + idle; $DV_HOST_POOL_GB, default min(24 GB, a quarter
    of the machine's RAM); 0 disables the pool) - beyond it a request gets a plain np.empty; idle blocks are kept only up
    to the total of the last four requests (a deblend_field call asks for three arrays) and are dropped when they have
    not been used for eight requests, so one large call does not pin its memory for the life of the process.
    host_pool_clear() drops every idle block at once.  Arrays below 64 MB are plain np.empty."""

    MIN_BYTES = 64 << 20
    KEEP_REQUESTS = 4          # idle bytes kept <= the total of this many most recent requests
    MAX_IDLE_AGE = 8           # ... and an idle block older than this many requests is dropped

    def __init__(self, cap_bytes: Optional[int] = None):
        if cap_bytes is None:
            try:
                cap_bytes = int(float(os.environ["DV_HOST_POOL_GB"]) * (1 << 30))
            except (KeyError, ValueError):
                cap_bytes = min(24 << 30, self._ram_bytes() // 4)
        self.cap = max(0, cap_bytes)
        self._lock = threading.Lock()
        self._idle: List[tuple] = []                       # (block, tick of its last use), least recently used first
        self._returned = collections.deque()               # blocks whose lease has died, not yet back on the idle list
        self._leased = 0                                   # bytes handed out and not yet returned
        self._recent = collections.deque(maxlen=self.KEEP_REQUESTS)
        self._tick = 0

    @staticmethod
    def _ram_bytes() -> int:
        try:
            return os.sysconf("SC_PAGE_SIZE") * os.sysconf("SC_PHYS_PAGES")
        except (ValueError, OSError, AttributeError):
            return 64 << 30

    def _give_back(self, block: np.ndarray):
        """finalizer of a lease (any thread, possibly inside empty() via the garbage collector): no lock taken here"""
        self._returned.append(block)

    def _drain(self):
        while True:
            try:
                block = self._returned.popleft()
            except IndexError:
                return
            self._leased -= block.nbytes
            self._idle.append((block, self._tick))

    def _trim(self, keep_bytes: int):
        """drops idle blocks that are too old, then the least recently used ones until at most keep_bytes stay idle"""
        self._idle = [(b, t) for b, t in self._idle if self._tick - t <= self.MAX_IDLE_AGE]
        total = sum(b.nbytes for b, _ in self._idle)
        while self._idle and total > keep_bytes:
            total -= self._idle.pop(0)[0].nbytes

    def empty(self, shape, dtype) -> np.ndarray:
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if nbytes < self.MIN_BYTES or nbytes > self.cap:
            return np.empty(shape, dtype)
        with self._lock:
            self._tick += 1
            self._drain()
            self._recent.append(nbytes)
            pick = -1
            for i, (b, _) in enumerate(self._idle):           # best fit among the idle blocks
                if b.nbytes >= nbytes and (pick < 0 or b.nbytes < self._idle[pick][0].nbytes):
                    pick = i
            if pick >= 0:
                block = self._idle.pop(pick)[0]
            else:
                idle = sum(b.nbytes for b, _ in self._idle)
                if self._leased + idle + nbytes > self.cap:   # make room among the idle blocks first
                    self._trim(max(0, self.cap - self._leased - nbytes))
                    idle = sum(b.nbytes for b, _ in self._idle)
                if self._leased + idle + nbytes > self.cap:
                    return np.empty(shape, dtype)             # everything tracked is in use: a plain array, not tracked
                block = np.empty(nbytes, np.uint8)
            self._leased += block.nbytes
            self._trim(sum(self._recent))
            lease = _Lease(block, nbytes)
            weakref.finalize(lease, self._give_back, block)
            out = np.asarray(lease).view(dtype).reshape(shape)  # the only references to `lease` are out's base chain
            del lease
            return out

    def stats(self) -> dict:
        with self._lock:
            self._drain()
            return {"cap": self.cap, "leased_bytes": self._leased, "idle_bytes": sum(b.nbytes for b, _ in self._idle),
                    "idle_blocks": len(self._idle)}

    def clear(self):
        """drops every idle block (leased ones belong to their holders and are freed when those let go)"""
        with self._lock:
            self._drain()
            self._idle = []


_host_pool = _HostPool()


def host_pool_clear():
    """Frees the idle blocks of the result-array pool (see _HostPool) - e.g. after the last deblend_field of a session."""
    _host_pool.clear()


def host_pool_stats() -> dict:
    return _host_pool.stats()


def _f32c(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {tuple(a.shape)}")
    return a


class Context:
    """One per process: selects the GPU, owns the HIP streams and the RCCL communicator.

    Lifetime: every Engine registers with its Context; close() destroys the live engines first (their buffers, events
    and pinned memory hang off the context's device and streams), then the communicator and the streams.  Contexts still
    open when the interpreter exits are closed by an atexit hook, i.e. BEFORE Python finalises modules in arbitrary
    order and before the C runtime runs the HIP runtime's own exit handlers - relying on __del__ there left models
    alive behind their context (SIGSEGV inside exit() under rocprofv3)."""

    _live: "weakref.WeakSet[Context]" = weakref.WeakSet()

    def __init__(self, device: int = 0, rank: int = 0, world: int = 1, unique_id: Optional[bytes] = None):
        self._h = C.c_void_p()
        self._engines: "weakref.WeakSet[Engine]" = weakref.WeakSet()
        self.group = None                 # host-side rendezvous of the job (debvader_amd.parallel.make_context)
        self._owns_group = False
        self.rank, self.world, self.device = rank, world, device
        idbuf = None
        if world > 1:
            if unique_id is None or len(unique_id) != _lib.DV_UNIQUE_ID_BYTES:
                raise ValueError("world > 1 needs rank 0's unique id (Context.unique_id())")
            idbuf = C.create_string_buffer(unique_id, _lib.DV_UNIQUE_ID_BYTES)
        check(lib.dv_ctx_create(device, rank, world, idbuf, C.byref(self._h)))
        Context._live.add(self)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(_lib.DV_UNIQUE_ID_BYTES)
        check(lib.dv_comm_unique_id(buf))
        return buf.raw

    def sync(self):
        check(lib.dv_ctx_sync(self._h))

    def comm_info(self) -> Dict:
        """What the RCCL communicator of this context really spans: {comm_ranks (ncclCommCount, 0 without one), comm_rank,
        device, bus_id (PCI), rehearsal (DV_DEBUG_FAKE_PEERS: a one-rank communicator although world > 1)}."""
        n, r, d, reh = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        bus = C.create_string_buffer(32)
        check(lib.dv_ctx_comm_info(self._h, C.byref(n), C.byref(r), C.byref(d), bus, 32, C.byref(reh)))
        return dict(comm_ranks=n.value, comm_rank=r.value, device=d.value, bus_id=bus.value.decode(),
                    rehearsal=bool(reh.value), world=self.world, rank=self.rank)

    def mem_info(self) -> Tuple[int, int]:
        """(free, total) bytes of device memory on this context's GPU (hipMemGetInfo)."""
        fr, tot = C.c_int64(), C.c_int64()
        check(lib.dv_ctx_mem_info(self._h, C.byref(fr), C.byref(tot)))
        return fr.value, tot.value

    def comm_prof(self, on: bool):
        """Time every collective on the comm stream and every wait of the main stream for one (dv_comm_prof_enable)."""
        check(lib.dv_comm_prof_enable(self._h, int(on)))

    def comm_prof_read(self) -> Dict:
        """{collectives, comm_ms, waits, exposed_ms} since the last read (synchronises)."""
        n1, n2, a, b = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        check(lib.dv_comm_prof_read(self._h, C.byref(n1), C.byref(a), C.byref(n2), C.byref(b)))
        return dict(collectives=n1.value, comm_ms=a.value, waits=n2.value, exposed_ms=b.value)

    def allreduce(self, values: Sequence[float]) -> np.ndarray:
        a = np.ascontiguousarray(values, dtype=np.float32)
        check(lib.dv_ctx_allreduce_host(self._h, _fp(a), a.size))
        return a

    # -- scene compositing (float64 host arrays, like the reference's numpy fields) --------------
    def scene_extract(self, field, starts, cutout_size: int) -> np.ndarray:
        """cutouts[i] = field[starts[i,0]:+cs, starts[i,1]:+cs, :] for a field (F, F, bands)."""
        field = np.ascontiguousarray(field, dtype=np.float64)
        starts = _i32_rows(starts, "cutout starts")
        if field.ndim != 3 or field.shape[0] != field.shape[1]:
            raise ValueError(f"expected a square field (F, F, bands), got {field.shape}")
        out = np.empty((starts.shape[0], cutout_size, cutout_size, field.shape[2]), np.float64)
        dp = C.POINTER(C.c_double)
        check(lib.dv_scene_extract(self._h, field.ctypes.data_as(dp), field.shape[0], field.shape[2],
                                   starts.ctypes.data_as(C.POINTER(C.c_int32)), starts.shape[0], int(cutout_size),
                                   out.ctypes.data_as(dp)))
        return out

    def scene_composite(self, field, stamps, positions, sign: float = 1.0) -> np.ndarray:
        """field + sign * sum_i shift(pad(stamps[i]), positions[i]) (scipy.ndimage.shift semantics), in object order."""
        out = np.array(field, dtype=np.float64, order="C", copy=True)
        stamps = np.ascontiguousarray(stamps, dtype=np.float64)
        positions = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 2)
        if out.ndim != 3 or out.shape[0] != out.shape[1]:
            raise ValueError(f"expected a square field (F, F, bands), got {out.shape}")
        if stamps.shape[0] == 0:
            return out
        if stamps.ndim != 4 or stamps.shape[1] != stamps.shape[2] or stamps.shape[3] != out.shape[2] \
                or stamps.shape[0] != positions.shape[0]:
            raise ValueError(f"stamps {stamps.shape} / positions {positions.shape} do not fit field {out.shape}")
        dp = C.POINTER(C.c_double)
        check(lib.dv_scene_composite(self._h, out.ctypes.data_as(dp), out.shape[0], out.shape[2],
                                     stamps.ctypes.data_as(dp), positions.ctypes.data_as(dp), stamps.shape[0],
                                     stamps.shape[1], float(sign)))
        return out

    FIT_CONVERGED, FIT_ON_BOUND, FIT_ITER_LIMIT, FIT_STALLED = 0, 1, 2, 3     # status codes of scene_fit_shifts

    def scene_fit_shifts(self, field_r, stamps_r, distances, shifts=None, bound: float = 3.0,
                         max_iter: int = 50) -> Dict[str, np.ndarray]:
        """Sub-pixel position fit of every galaxy on the r band (deblend_cutout/optimization.py, batched on the GPU).

        field_r (F, F), stamps_r (N, cs, cs), distances (N, 2) {row, column} to the centre.  Galaxy i minimises
        J(s) = mean over the field of (field_r - shift(shift(pad(stamps_r[i]), distances[i]), s))^2 over s in
        [-bound, bound]^2, started from shifts[i] (zeros by default), with scipy.ndimage.shift semantics.
        Returns {shifts (N, 2), objective (N,) J at them, iters (N,), status (N,): FIT_CONVERGED, FIT_ON_BOUND,
        FIT_ITER_LIMIT or FIT_STALLED (no damped step lowered J)}.  max_iter = 0 evaluates J at the given shifts."""
        field_r = np.ascontiguousarray(field_r, dtype=np.float64)
        stamps_r = np.ascontiguousarray(stamps_r, dtype=np.float64)
        dist = np.ascontiguousarray(distances, dtype=np.float64)
        if field_r.ndim != 2 or field_r.shape[0] != field_r.shape[1] or field_r.shape[0] < 2:
            raise ValueError(f"expected a square r-band field (F, F), got {field_r.shape}")
        if stamps_r.ndim != 3 or stamps_r.shape[1] != stamps_r.shape[2] or stamps_r.shape[1] > field_r.shape[0]:
            raise ValueError(f"expected square r-band stamps (N, cs, cs) with cs <= {field_r.shape[0]}, got {stamps_r.shape}")
        n = stamps_r.shape[0]
        if dist.shape != (n, 2):
            raise ValueError(f"expected distances ({n}, 2), got {dist.shape}")
        out = np.zeros((n, 2), np.float64) if shifts is None else np.array(shifts, dtype=np.float64, order="C", copy=True)
        if out.shape != (n, 2):
            raise ValueError(f"expected shifts ({n}, 2), got {out.shape}")
        if not (np.isfinite(bound) and bound >= 0) or int(max_iter) < 0:
            raise ValueError(f"bound must be finite and >= 0, max_iter >= 0 (got {bound}, {max_iter})")
        obj = np.zeros(n, np.float64)
        iters = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        if n:
            dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
            check(lib.dv_scene_fit_shifts(self._h, field_r.ctypes.data_as(dp), field_r.shape[0], stamps_r.ctypes.data_as(dp),
                                          n, stamps_r.shape[1], dist.ctypes.data_as(dp), float(bound), int(max_iter),
                                          out.ctypes.data_as(dp), obj.ctypes.data_as(dp), iters.ctypes.data_as(ip),
                                          status.ctypes.data_as(ip)))
        return dict(shifts=out, objective=obj, iters=iters, status=status)

    def scene_fit_shifts_fields(self, fields_r, stamps_r, distances, field_ptr, shifts=None, bound: float = 3.0,
                                max_iter: int = 50) -> Dict[str, np.ndarray]:
        """scene_fit_shifts for the galaxies of M fields in one engine call (dv_scene_fit_shifts_fields): fields_r (M, F, F),
        stamps_r (N, cs, cs), distances (N, 2), field_ptr (M + 1,) - galaxies field_ptr[m]:field_ptr[m + 1] are fitted against
        field m.  Same result dictionary; every galaxy gets what scene_fit_shifts gives it on its own field, bit for bit."""
        fields_r = np.ascontiguousarray(fields_r, dtype=np.float64)
        stamps_r = np.ascontiguousarray(stamps_r, dtype=np.float64)
        dist = np.ascontiguousarray(distances, dtype=np.float64)
        if fields_r.ndim != 3 or fields_r.shape[1] != fields_r.shape[2] or fields_r.shape[1] < 2:
            raise ValueError(f"expected square r-band fields (M, F, F), got {fields_r.shape}")
        if stamps_r.ndim != 3 or stamps_r.shape[1] != stamps_r.shape[2] or stamps_r.shape[1] > fields_r.shape[1]:
            raise ValueError(f"expected square r-band stamps (N, cs, cs) with cs <= {fields_r.shape[1]}, got {stamps_r.shape}")
        n = stamps_r.shape[0]
        if dist.shape != (n, 2):
            raise ValueError(f"expected distances ({n}, 2), got {dist.shape}")
        fp = check_field_ptr(field_ptr, fields_r.shape[0], n)
        out = np.zeros((n, 2), np.float64) if shifts is None else np.array(shifts, dtype=np.float64, order="C", copy=True)
        if out.shape != (n, 2):
            raise ValueError(f"expected shifts ({n}, 2), got {out.shape}")
        if not (np.isfinite(bound) and bound >= 0) or int(max_iter) < 0:
            raise ValueError(f"bound must be finite and >= 0, max_iter >= 0 (got {bound}, {max_iter})")
        obj = np.zeros(n, np.float64)
        iters = np.zeros(n, np.int32)
        status = np.zeros(n, np.int32)
        if n:
            dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
            check(lib.dv_scene_fit_shifts_fields(self._h, fields_r.ctypes.data_as(dp), fields_r.shape[0], fields_r.shape[1],
                                                 stamps_r.ctypes.data_as(dp), fp.ctypes.data_as(C.POINTER(C.c_int64)), n,
                                                 stamps_r.shape[1], dist.ctypes.data_as(dp), float(bound), int(max_iter),
                                                 out.ctypes.data_as(dp), obj.ctypes.data_as(dp), iters.ctypes.data_as(ip),
                                                 status.ctypes.data_as(ip)))
        return dict(shifts=out, objective=obj, iters=iters, status=status)

    MEASURE_CONVERGED, MEASURE_ITER_LIMIT, MEASURE_FAILED = 0, 2, 3           # status codes of scene_measure

    def scene_measure(self, mean, stddev=None, band: int = 2, sigma0: float = 3.0, tol: float = 1e-10,
                      max_iter: int = 200) -> Dict[str, np.ndarray]:
        """Catalogue measurement of N stamps on the GPU (dv_scene_measure): mean, stddev (N, cs, cs,
        bands) - the network's mean and stddev stamps, taken as float32.  Returns {"flux" (N, bands): the sum of every
        band's mean stamp, ["flux_err" (N, bands): sqrt of the sum of the squared stddev stamp, when stddev is given],
        "shape" (N, 5): {row, col, Mrr, Mrc, Mcc}, the adaptive moments of band `band` (rows and columns counted from the
        stamp's pixel 0), "iters" (N,), "status" (N,): MEASURE_CONVERGED, MEASURE_ITER_LIMIT or MEASURE_FAILED (degenerate
        moments, no positive weighted flux, or a centroid that left the stamp)}, float64 throughout."""
        mean, stddev, par = check_measure_args(mean, stddev, band, sigma0, tol, max_iter)
        n, cs, nb = mean.shape[0], mean.shape[1], mean.shape[3]
        out = {"flux": np.zeros((n, nb), np.float64)}
        if stddev is not None:
            out["flux_err"] = np.zeros((n, nb), np.float64)
        out.update(shape=np.zeros((n, 5), np.float64), iters=np.zeros(n, np.int32), status=np.zeros(n, np.int32))
        if n:
            check(lib.dv_scene_measure(self._h, _fp(mean), _fp(stddev), n, cs, nb, C.byref(par), _dp(out["flux"]),
                                       _dp(out.get("flux_err")), _dp(out["shape"]), _ip(out["iters"]), _ip(out["status"])))
        return out

    def scene_measure_mc(self, samples, band: int = 2, sigma0: float = 3.0, tol: float = 1e-10, max_iter: int = 200,
                         keep_samples: bool = False, _chunk=None) -> Dict[str, np.ndarray]:
        """Monte-Carlo catalogue of N galaxies on the GPU (dv_scene_measure_mc): samples (S, N, cs, cs,
        bands), S stochastic decodes of every galaxy, taken as float32.  Every sample is measured as scene_measure does
        without a stddev stamp; per galaxy the rows are folded in sample order (Welford) into {"flux_mc_mean", "flux_mc_std"
        (N, bands): over all S samples, "shape_mc_mean", "shape_mc_std" (N, 8): {row, col, Mrr, Mrc, Mcc, sigma, e1, e2}
        (MC_SHAPE_NAMES) over the accepted samples - status 0, det M > 0, trace > 0 -, "n_ok" (N,): how many those were
        (0: NaN, 1: std 0)}, float64, std in the population form.  keep_samples=True adds the per-sample rows "sample_flux"
        (N, S, bands), "sample_shape" (N, S, 5) and "sample_status" (N, S).  A galaxy's result depends on its own samples
        only.  (_chunk: galaxies per library call, for tests.)"""
        samples, par = check_measure_mc_args(samples, band, sigma0, tol, max_iter)
        S, n, cs, nb = samples.shape[0], samples.shape[1], samples.shape[2], samples.shape[4]
        out, ptrs = _measure_mc_out(n, nb, S, keep_samples)
        if _chunk is not None and 0 < int(_chunk) < n:
            parts = [self.scene_measure_mc(samples[:, g:g + int(_chunk)], band, sigma0, tol, max_iter, keep_samples)
                     for g in range(0, n, int(_chunk))]
            return {k: np.concatenate([q[k] for q in parts]) for k in out}
        if n:
            check(lib.dv_scene_measure_mc(self._h, _fp(samples), S, n, cs, nb, C.byref(par), *ptrs))
        return out

    def scene_blend(self, stamps, shape, status, places, model_fields, data_fields=None, field_ptr=None,
                    band: int = 2) -> Dict[str, np.ndarray]:
        """Blendedness sums of N galaxies on the GPU (dv_scene_blend): stamps (N, cs, cs, bands), the
        mean stamps taken as float32; shape (N, 5) and status (N,), their scene_measure rows; places (N, 2), the field
        position (row, col) of every stamp's top-left corner; model_fields (M, F, F, bands), the composited mean fields;
        data_fields the observed fields of the same shape, or None; field_ptr (M + 1,): stamps field_ptr[m]:field_ptr[m + 1]
        lie in field m (None: one field holds them all).  Returns {"blend" (N, 4): {W, A, Bm, Bd} = the sums of g, g * stamp,
        g * model field, g * data field over the stamp's pixels inside the field, g the Gaussian of the galaxy's adaptive
        moments in band `band`; "npix" (N,): the pixels summed}.  A row whose status is neither 0 nor 2, whose shape is not
        finite or whose det M is not above 1e-6 gets four NaN and npix -1; without data_fields Bd is NaN."""
        stamps = np.ascontiguousarray(stamps, dtype=np.float32)
        if stamps.ndim != 4 or stamps.shape[1] != stamps.shape[2]:
            raise ValueError(f"expected square stamps (N, cs, cs, bands), got {stamps.shape}")
        n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
        model = np.ascontiguousarray(model_fields, dtype=np.float64)
        if model.ndim != 4 or model.shape[1] != model.shape[2] or model.shape[3] != nb:
            raise ValueError(f"expected model fields (M, F, F, {nb}), got {model.shape}")
        data = None
        if data_fields is not None:
            data = np.ascontiguousarray(data_fields, dtype=np.float64)
            if data.shape != model.shape:
                raise ValueError(f"expected data fields {model.shape}, got {data.shape}")
        shape = np.ascontiguousarray(shape, dtype=np.float64)
        status = np.ascontiguousarray(status, dtype=np.int32)
        places = _i32_rows(places, "stamp placements")
        if shape.shape != (n, 5) or status.shape != (n,) or places.shape != (n, 2):
            raise ValueError(f"expected shape ({n}, 5), status ({n},) and places ({n}, 2), got {shape.shape}, {status.shape}, "
                             f"{places.shape}")
        if not 0 <= int(band) < nb:
            raise ValueError(f"band {band} asked for, the stamps have bands 0 .. {nb - 1}")
        M = model.shape[0]
        if field_ptr is None:
            if M != 1:
                raise ValueError(f"field_ptr is needed with {M} fields")
            field_ptr = [0, n]
        fp = check_field_ptr(field_ptr, M, n)
        out = dict(blend=np.zeros((n, 4), np.float64), npix=np.zeros(n, np.int32))
        if n:
            check(lib.dv_scene_blend(self._h, _fp(stamps), _dp(shape), _ip(status), _ip(places),
                                     fp.ctypes.data_as(C.POINTER(C.c_int64)), n, cs, nb, int(band), _dp(model), _dp(data), M,
                                     model.shape[1], _dp(out["blend"]), _ip(out["npix"])))
        return out

    REGAUSS_INELIGIBLE, REGAUSS_NO_PSF, REGAUSS_UNRESOLVED = 4, 5, 6          # status codes scene_regauss adds to scene_measure's

    def scene_regauss(self, stamps, shape, status, psf, psf_index=None, band: int = 2, psf_sigma0: float = 2.0,
                      tol: float = 1e-10, max_iter: int = 200) -> Dict[str, np.ndarray]:
        """PSF-corrected moments of N galaxies on the GPU by re-Gaussianization (dv_scene_regauss):
        stamps (N, cs, cs, bands), the mean stamps taken as float32; shape (N, 5) and status (N,), their scene_measure rows in
        band `band`; psf (K, ps, ps) float64 PSF images (or one (ps, ps)), psf_index (N,) the PSF of every galaxy (None: PSF
        0).  Returns {"regauss" (N, 6): {row', col', Mrr', Mrc', Mcc', rho4} - the adaptive moments and the kurtosis of the
        galaxy's band plane less the part of it that the PSF's departure from its own best Gaussian accounts for -,
        "regauss_iters", "regauss_status" (N,): 0 / 2 / 3 as scene_measure, REGAUSS_INELIGIBLE (the row's status is 3, a value
        is not finite or det M <= 1e-6), REGAUSS_NO_PSF (psf_index outside 0 .. K - 1, or a PSF that is not usable),
        REGAUSS_UNRESOLVED (M - M_P is not positive definite) - the last three with six NaN and 0 iterations; "psf_shape"
        (K, 5), "psf_aux" (K, 3): {A_P, sum Q, psf_rho4}, "psf_iters", "psf_status" (K,): the PSFs' own adaptive moments from
        the width psf_sigma0}.  The corrected moments are regauss[:, 2:5] - psf_shape[psf_index, 2:5]
        (debvader_amd.measure.measurement.psf_records derives sigma, e1, e2 and the resolution from them)."""
        stamps = np.ascontiguousarray(stamps, dtype=np.float32)
        if stamps.ndim != 4 or stamps.shape[1] != stamps.shape[2] or stamps.shape[1] < 1 or stamps.shape[3] < 1:
            raise ValueError(f"expected square stamps (N, cs, cs, bands), got {stamps.shape}")
        n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
        if cs > REGAUSS_MAX_STAMP:
            raise ValueError(f"stamps of {cs} pixels: the PSF correction takes at most {REGAUSS_MAX_STAMP}")
        shape = np.ascontiguousarray(shape, dtype=np.float64)
        status = np.ascontiguousarray(status, dtype=np.int32)
        if shape.shape != (n, 5) or status.shape != (n,):
            raise ValueError(f"expected shape ({n}, 5) and status ({n},), got {shape.shape}, {status.shape}")
        par = measure_params(band, 1.0, tol, max_iter, nb)
        psf, index = check_psf_args(psf, psf_index, n, psf_sigma0)
        K, ps = psf.shape[0], psf.shape[1]
        out, ptrs = _regauss_out(n, K)
        check(lib.dv_scene_regauss(self._h, _fp(stamps), _dp(shape), _ip(status), _ip(index), n, cs, nb, par.band, _dp(psf), K, ps,
                                   float(psf_sigma0), par.tol, par.max_iter, *ptrs))
        return out

    APER_OK, APER_INELIGIBLE, APER_NO_KRON = 0, 4, 7          # aper_status of scene_aperture
    APER_FLAG_AUTO_TRUNCATED, APER_FLAG_LIMIT_TRUNCATED, APER_FLAG_KRON_MIN = 1 << 8, 1 << 9, 1 << 10   # (bit k < 8: circle k truncated)

    def scene_aperture(self, mean, shape, status, stddev=None, radii=(3.0, 5.0, 8.0), fractions=(0.2, 0.5, 0.8), band: int = 2,
                       subsample: int = 5, kron_factor: float = 2.5, kron_min: float = 3.5, kron_limit: float = 6.0,
                       bisect_iters: int = 32) -> Dict[str, np.ndarray]:
        """Aperture photometry of N galaxies on the GPU (dv_scene_aperture): mean, stddev (N, cs, cs,
        bands) the network's stamps, taken as float32 (stddev optional); shape (N, 5) and status (N,) their scene_measure rows
        in band `band`.  Returns {"ap_flux", ["ap_flux_err"] (N, K, bands): the flux in K circles of `radii` pixels about the
        measured centroid, pixels weighted by the share of their subsample x subsample sub-pixels inside; "ap_area" (N, K);
        "flux_auto", ["flux_auto_err"] (N, bands): the flux in the Kron ellipse; "kron" (N, 3): {r1 - the first radial moment
        of band `band` in units of the moment ellipse, taken inside kron_limit -, rho_auto = max(kron_factor r1, kron_min),
        auto_area}; "flux_rho" (N, J): the ellipse radii that hold `fractions` of flux_auto[band]; "aper_flags" (N,): bit k
        circle k leaves the stamp, APER_FLAG_AUTO_TRUNCATED, APER_FLAG_LIMIT_TRUNCATED, APER_FLAG_KRON_MIN; "aper_status"
        (N,): APER_OK, APER_INELIGIBLE (the row's status is 3, a value is not finite or det M <= 1e-6: every float NaN),
        APER_NO_KRON (no positive flux inside kron_limit: the Kron outputs NaN, the circles given)}, float64 throughout."""
        mean, stddev, mpar = check_measure_args(mean, stddev, band, 1.0, 1.0, 0)
        n, cs, nb = mean.shape[0], mean.shape[1], mean.shape[3]
        shape = np.ascontiguousarray(shape, dtype=np.float64)
        status = np.ascontiguousarray(status, dtype=np.int32)
        if shape.shape != (n, 5) or status.shape != (n,):
            raise ValueError(f"expected shape ({n}, 5) and status ({n},), got {shape.shape}, {status.shape}")
        par = aperture_params(radii, fractions, subsample, kron_factor, kron_min, kron_limit, bisect_iters)
        out, ptrs = _aperture_out(n, nb, par, err=stddev is not None)
        if n:
            check(lib.dv_scene_aperture(self._h, _fp(mean), _fp(stddev), _dp(shape), _ip(status), n, cs, nb, mpar.band,
                                        C.byref(par), *ptrs))
        return out

    def scene_aperture_fields(self, shape, status, places, kron, aper_status, model_fields, data_fields=None, field_ptr=None, *,
                              cutout_size: int, radii=(3.0, 5.0, 8.0), subsample: int = 5) -> Dict[str, np.ndarray]:
        """The apertures of scene_aperture on the fields the galaxies lie in (dv_scene_aperture_fields, DESIGN.md section
        7p): shape (N, 5) and status (N,) the scene_measure rows, kron (N, 3) and aper_status (N,) the scene_aperture rows
        measured with the same `radii` and `subsample` on stamps of cutout_size pixels; places (N, 2) the field position
        (row, col) of every stamp's top-left corner; model_fields (M, F, F, bands) the composited mean fields, data_fields
        the observed fields of the same shape, or None; field_ptr (M + 1,): galaxies field_ptr[m]:field_ptr[m + 1] lie in
        field m (None: one field holds them all).  No stamp is an input.  Returns {"ap_model_sum", "ap_data_sum" (N, K,
        bands): the sums of w * model field and w * data field over the stamp pixels of circle k that lie inside the field, w
        the sub-pixel weight of scene_aperture; "ap_field_area" (N, K): the sum of w over those pixels; "auto_model_sum",
        "auto_data_sum" (N, bands), "auto_field_area" (N,): the same in the Kron ellipse of radius kron[:, 1]}.  A row with
        aper_status APER_INELIGIBLE is NaN throughout, a row with APER_NO_KRON in the three auto_ outputs; without
        data_fields the two _data_sum outputs are NaN; a stamp wholly outside its field gives zeros."""
        model = np.ascontiguousarray(model_fields, dtype=np.float64)
        if model.ndim != 4 or model.shape[1] != model.shape[2] or model.shape[3] < 1:
            raise ValueError(f"expected model fields (M, F, F, bands), got {model.shape}")
        M, nb = model.shape[0], model.shape[3]
        data = None
        if data_fields is not None:
            data = np.ascontiguousarray(data_fields, dtype=np.float64)
            if data.shape != model.shape:
                raise ValueError(f"expected data fields {model.shape}, got {data.shape}")
        shape = np.ascontiguousarray(shape, dtype=np.float64)
        status = np.ascontiguousarray(status, dtype=np.int32)
        kron = np.ascontiguousarray(kron, dtype=np.float64)
        aper_status = np.ascontiguousarray(aper_status, dtype=np.int32)
        places = _i32_rows(places, "stamp placements")
        n = status.shape[0] if status.ndim == 1 else -1
        if shape.shape != (n, 5) or places.shape != (n, 2) or kron.shape != (n, 3) or aper_status.shape != (n,):
            raise ValueError(f"expected shape (N, 5), status (N,), places (N, 2), kron (N, 3) and aper_status (N,), got "
                             f"{shape.shape}, {status.shape}, {places.shape}, {kron.shape}, {aper_status.shape}")
        cs = int(cutout_size)
        if cs != cutout_size or cs < 1:
            raise ValueError(f"cutout_size must be a positive integer (got {cutout_size})")
        if field_ptr is None:
            if M != 1:
                raise ValueError(f"field_ptr is needed with {M} fields")
            field_ptr = [0, n]
        fp = check_field_ptr(field_ptr, M, n)
        par = aperture_params(radii, (), subsample)
        out, ptrs = _aperture_field_out(n, nb, par)
        if n:
            check(lib.dv_scene_aperture_fields(self._h, _dp(shape), _ip(status), _ip(places),
                                               fp.ctypes.data_as(C.POINTER(C.c_int64)), _dp(kron), _ip(aper_status), n, cs, nb,
                                               _dp(model), _dp(data), M, model.shape[1], C.byref(par), *ptrs))
        return out

    FIT_INELIGIBLE, FIT_DROPPED = 4, 5                 # fit_status of scene_fit_flux beside 0 (fitted)

    def scene_fit_flux(self, stamps, places, data_fields, field_ptr=None, min_pivot: float = 1e-8,
                       scratch_bytes: int = 256 << 20, weight_fields=None) -> Dict[str, np.ndarray]:
        """The simultaneous flux fit of the deblended models to the observed field on the GPU (dv_scene_fit_flux, DESIGN.md
        section 7q): stamps (N, cs, cs, bands), the mean stamps taken as float32; places (N, 2), the field position (row, col)
        of every stamp's top-left corner; data_fields (M, F, F, bands), the observed fields; field_ptr (M + 1,): stamps
        field_ptr[m]:field_ptr[m + 1] lie in field m (None: one field holds them all).  Per field and band the amplitudes a
        that minimise |D - sum a_i P_i|^2 over the pixels inside the field, the shapes P_i held fixed.  Returns, all (N,
        bands): {"fit_scale": a; "fit_var": the diagonal of the inverse Gram matrix of the fitted galaxies; "fit_gram": G_ii
        = sum P_i^2; "fit_proj": h_i = sum P_i D; "fit_status": 0 fitted, FIT_INELIGIBLE G_ii not positive (scale and var
        NaN), FIT_DROPPED the galaxy cannot be told from earlier ones of its field - pivot <= min_pivot G_ii - and keeps the
        network's amplitude (scale 1, var NaN)}.  A field of more than 1024 galaxies, or whose bands x n x n doubles exceed
        scratch_bytes, is refused.
        weight_fields (M, F, F, bands), or (F, F, bands) for one field: the weighted fit (dv_scene_fit_flux_weighted, DESIGN.md
        section 7s).  W is the inverse variance of every pixel; a pixel counts iff 0 < W < inf, every other weight masks it and
        nothing under it - a NaN in the data included - reaches a sum.  G_ij = sum W P_i P_j and h_i = sum W P_i D over the
        counting pixels, fit_var is the variance of fit_scale, and the dictionary gains "fit_chi2", the chi-square of the
        refitted scene under the galaxy's own counting pixels (NaN with FIT_INELIGIBLE), and "fit_npix" (int32), their number.
        The five shared arrays of W = 1 everywhere have the bits of the unweighted call."""
        stamps = np.ascontiguousarray(stamps, dtype=np.float32)
        if stamps.ndim != 4 or stamps.shape[1] != stamps.shape[2]:
            raise ValueError(f"expected square stamps (N, cs, cs, bands), got {stamps.shape}")
        n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
        data = np.ascontiguousarray(data_fields, dtype=np.float64)
        if data.ndim != 4 or data.shape[1] != data.shape[2] or data.shape[3] != nb:
            raise ValueError(f"expected data fields (M, F, F, {nb}), got {data.shape}")
        places = _i32_rows(places, "stamp placements")
        if places.shape != (n, 2):
            raise ValueError(f"expected places ({n}, 2), got {places.shape}")
        M = data.shape[0]
        if field_ptr is None:
            if M != 1:
                raise ValueError(f"field_ptr is needed with {M} fields")
            field_ptr = [0, n]
        fp = check_field_ptr(field_ptr, M, n)
        par = fit_flux_params(min_pivot, scratch_bytes)
        weights = None if weight_fields is None else check_fit_weights(weight_fields, data.shape)
        out, ptrs = _fit_flux_out(n, nb, weights is not None)
        if n and weights is not None:
            check(lib.dv_scene_fit_flux_weighted(self._h, _fp(stamps), _ip(places), fp.ctypes.data_as(C.POINTER(C.c_int64)), n,
                                                 cs, nb, _dp(data), _dp(weights), M, data.shape[1], C.byref(par), *ptrs))
        elif n:
            check(lib.dv_scene_fit_flux(self._h, _fp(stamps), _ip(places), fp.ctypes.data_as(C.POINTER(C.c_int64)), n, cs, nb,
                                        _dp(data), M, data.shape[1], C.byref(par), *ptrs))
        return out

    def scene_moments_fields(self, stamps, places, model_fields, data_fields, weight_fields=None, field_ptr=None, band: int = 2,
                             sigma0: float = 3.0, tol: float = 1e-10, max_iter: int = 200) -> Dict[str, np.ndarray]:
        """Adaptive moments on the observed field with the neighbours subtracted (dv_scene_moments_fields, DESIGN.md section
        7x): stamps (N, cs, cs, bands), the mean stamps taken as float32; places (N, 2), the field position (row, col) of every
        stamp's top-left corner; model_fields (M, F, F, bands), the composited mean fields T; data_fields of the same shape,
        the observed fields D; weight_fields of the same shape or None - a mask only: a pixel counts iff it lies inside the
        field and 0 < W < inf; field_ptr (M + 1,): stamps field_ptr[m]:field_ptr[m + 1] lie in field m (None: one field holds
        them all).  Per galaxy the child image C = (D - T) + stamp where the pixel counts and the stamp elsewhere.  Returns
        {"flux_data" (N, bands): the sum of every band of C; "npix_data" (N, bands) int32: the counting pixels; "shape_data"
        (N, 5), "iters_data", "status_data" (N,): scene_measure's adaptive moments of band `band` of C}.  Where D has the bits
        of T every output has the bits of scene_measure on the stamps."""
        stamps, places, model, fp = _fit_scene_inputs(stamps, places, model_fields, field_ptr)
        n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
        if cs < 1 or nb < 1:
            raise ValueError(f"expected square stamps (N, cs, cs, bands), got {stamps.shape}")
        if cs > MEASURE_MAX_STAMP:
            raise ValueError(f"stamps of {cs} pixels: the measurement takes at most {MEASURE_MAX_STAMP}")
        data = np.ascontiguousarray(data_fields, dtype=np.float64)
        if data.shape != model.shape:
            raise ValueError(f"expected data fields {model.shape}, got {data.shape}")
        weights = None if weight_fields is None else check_fit_weights(weight_fields, model.shape)
        par = measure_params(band, sigma0, tol, max_iter, nb)
        out, ptrs = _moments_data_out(n, nb)
        if n:
            check(lib.dv_scene_moments_fields(self._h, _fp(stamps), _ip(places), fp.ctypes.data_as(C.POINTER(C.c_int64)), n, cs,
                                              nb, _dp(model), _dp(data), None if weights is None else _dp(weights),
                                              model.shape[0], model.shape[1], C.byref(par), *ptrs))
        return out

    def scene_fit_flux_groups(self, stamps, places, data_fields, field_ptr=None, min_pivot: float = 1e-8,
                              scratch_bytes: int = 256 << 20, weight_fields=None) -> Dict[str, np.ndarray]:
        """scene_fit_flux by blend groups (dv_scene_fit_flux_groups): the connected components of the
        overlap graph of every field - two galaxies are adjacent iff their stamp rectangles, clipped to the field, intersect -
        are found on the GPU and each is solved on its own.  A field may hold any number of galaxies; a group of more than 1024,
        or whose bands x n_g x n_g doubles exceed scratch_bytes, is refused by name.  Arguments and the dictionary are
        scene_fit_flux's, with weight_fields or without, with the bits of that call wherever it takes the field; two more
        arrays (N,) int32: "fit_group", the smallest row of the galaxy's group counted from the first row of its field, and
        "fit_group_size", the members of that group."""
        stamps, places, data, fp = _fit_scene_inputs(stamps, places, data_fields, field_ptr)
        n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
        par = fit_flux_params(min_pivot, scratch_bytes)
        weights = None if weight_fields is None else check_fit_weights(weight_fields, data.shape)
        out, ptrs = _fit_flux_out(n, nb, weights is not None)
        if weights is None:
            ptrs += [None, None]
        out["fit_group"], out["fit_group_size"] = np.zeros(n, np.int32), np.zeros(n, np.int32)
        if n:
            check(lib.dv_scene_fit_flux_groups(self._h, _fp(stamps), _ip(places), fp.ctypes.data_as(C.POINTER(C.c_int64)), n, cs,
                                               nb, _dp(data), data.shape[0], data.shape[1], C.byref(par),
                                               None if weights is None else _dp(weights), *ptrs, _ip(out["fit_group"]),
                                               _ip(out["fit_group_size"])))
        return out

    def scene_fit_groups(self, places, cutout_size: int, field_size: int, field_ptr=None, lists: bool = False) -> Dict[str, np.ndarray]:
        """The blend groups of scene_fit_flux_groups from the placements alone (dv_scene_fit_groups): places (N, 2), stamps of
        cutout_size pixels in fields of field_size; field_ptr (M + 1,), None: one field.  No fit, no limit on a group.  Returns
        {"fit_group", "fit_group_size"} (N,) int32 and, with lists=True, the lists the fit works from in rows of the call:
        "pairs" (n_pairs, 2), the adjacent (i, j <= i) sorted by i and then j, and the CSR adjacency "adj_ptr" (N + 1,) / "adj"
        with ascending lists."""
        places = _i32_rows(places, "stamp placements") if len(places) else np.zeros((0, 2), np.int32)
        n = places.shape[0]
        fp = check_field_ptr([0, n] if field_ptr is None else field_ptr, 1 if field_ptr is None else len(field_ptr) - 1, n)
        M = fp.shape[0] - 1
        out = dict(fit_group=np.zeros(n, np.int32), fit_group_size=np.zeros(n, np.int32))
        np_, na = C.c_int64(0), C.c_int64(0)
        args = [self._h, _ip(places), fp.ctypes.data_as(C.POINTER(C.c_int64)), n, int(cutout_size), M, int(field_size),
                _ip(out["fit_group"]), _ip(out["fit_group_size"])]
        check(lib.dv_scene_fit_groups(*args, 0, C.byref(np_), None, 0, C.byref(na), None, None))
        if lists:
            out.update(pairs=np.zeros((np_.value, 2), np.int32), adj_ptr=np.zeros(n + 1, np.int32), adj=np.zeros(na.value, np.int32))
            check(lib.dv_scene_fit_groups(*args, np_.value, C.byref(np_), _ip(out["pairs"]), na.value, C.byref(na),
                                          _ip(out["adj_ptr"]), _ip(out["adj"])))
        return out

    def scene_fit_flux_gram(self, stamps, places, data_field) -> Dict[str, np.ndarray]:
        """Step 1 of scene_fit_flux for the galaxies of one field (dv_scene_fit_flux_gram): stamps (n, cs, cs, bands), places
        (n, 2), data_field (F, F, bands).  Returns {"gram" (bands, n, n): G_ij = sum P_i P_j over the field pixels both
        stamps cover at [b, i, j] for j <= i, 0.0 above the diagonal; "proj" (n, bands): h_i = sum P_i D} with the bits the
        fit works on."""
        stamps = np.ascontiguousarray(stamps, dtype=np.float32)
        if stamps.ndim != 4 or stamps.shape[1] != stamps.shape[2]:
            raise ValueError(f"expected square stamps (n, cs, cs, bands), got {stamps.shape}")
        n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
        data = np.ascontiguousarray(data_field, dtype=np.float64)
        if data.ndim != 3 or data.shape[0] != data.shape[1] or data.shape[2] != nb:
            raise ValueError(f"expected one data field (F, F, {nb}), got {data.shape}")
        places = _i32_rows(places, "stamp placements")
        if places.shape != (n, 2):
            raise ValueError(f"expected places ({n}, 2), got {places.shape}")
        if n > FIT_FLUX_MAX_N:
            raise ValueError(f"{n} galaxies in one field, the dense flux fit takes at most {FIT_FLUX_MAX_N}")
        out = dict(gram=np.zeros((nb, n, n), np.float64), proj=np.zeros((n, nb), np.float64))
        if n:
            check(lib.dv_scene_fit_flux_gram(self._h, _fp(stamps), _ip(places), n, cs, nb, _dp(data), data.shape[0],
                                             _dp(out["gram"]), _dp(out["proj"])))
        return out

    def scene_fit_flux_sky(self, stamps, places, data_fields, field_ptr=None, sky_order: int = 0, weight_fields=None,
                           min_pivot: float = 1e-8, scratch_bytes: int = 256 << 20) -> Dict[str, np.ndarray]:
        """scene_fit_flux with a sky background fitted jointly (dv_scene_fit_flux_sky): per field and
        band q more unknowns beside the amplitudes - sky_order 0: a constant (q = 1); 1: a plane (q = 3) in the basis B_0 = 1,
        B_1 = (2 r - F + 1) / F, B_2 = (2 c - F + 1) / F of the field pixel (r, c) - fitted to ALL pixels of the field (with
        weight_fields: the counting ones).  The arguments are scene_fit_flux's.  Returns its dictionary ("fit_chi2" and
        "fit_npix" with weight_fields only; fit_var now carries the covariance with the sky; fit_status, fit_gram and fit_proj
        have the bits of the fit without sky) plus, per field: {"sky_coef" (M, bands, q); "sky_cov" (M, bands, q, q): the
        lower-right block of the inverse of the bordered matrix, NaN in the rows and columns of terms that are not kept;
        "sky_status" (M, bands, q) int32: 0 fitted, FIT_INELIGIBLE the field has no counting pixel (coefficient NaN),
        FIT_DROPPED the term cannot be told from the unknowns before it and is exactly 0.0; "sky_npix" (M, bands) int64: the
        counting pixels of the field}.  A field without galaxies is still solved.  Unweighted, a non-finite pixel of a data
        field anywhere reaches every galaxy of that field through the sky: mask it with weight_fields.  The scratch of a
        field is bands x (n + q) x (n + q) doubles."""
        stamps, places, data, fp = _fit_scene_inputs(stamps, places, data_fields, field_ptr)
        n, cs, nb, M = stamps.shape[0], stamps.shape[1], stamps.shape[3], data.shape[0]
        q = sky_terms(sky_order)
        par = fit_flux_params(min_pivot, scratch_bytes)
        weights = None if weight_fields is None else check_fit_weights(weight_fields, data.shape)
        out, ptrs = _fit_flux_out(n, nb, weights is not None)
        if weights is None:
            ptrs += [None, None]
        sky, sky_ptrs = _fit_sky_out(M, nb, q)
        out.update(sky)
        if M:
            check(lib.dv_scene_fit_flux_sky(self._h, _fp(stamps), _ip(places), fp.ctypes.data_as(C.POINTER(C.c_int64)), n, cs, nb,
                                            _dp(data), None if weights is None else _dp(weights), M, data.shape[1], C.byref(par),
                                            int(sky_order), *ptrs, *sky_ptrs))
        return out

    def scene_fit_flux_nonneg(self, stamps, places, data_fields, field_ptr=None, sky_order=None, weight_fields=None,
                              min_pivot: float = 1e-8, max_iter: int = 100, scratch_bytes: int = 256 << 20) -> Dict[str, np.ndarray]:
        """scene_fit_flux / scene_fit_flux_sky with the amplitudes constrained to be >= 0 (dv_scene_fit_flux_nonneg, DESIGN.md
        section 7u): the same quadratic minimised subject to a_i >= 0 for every galaxy, the sky (sky_order None: none; 0 a
        constant, 1 a plane) left free, by block principal pivoting on the GPU - at most max_iter factorisations per field
        and band.  The arguments are scene_fit_flux_sky's.  Returns the dictionary of the call without the constraint -
        "fit_scale" is exactly +0.0 where clamped, "fit_var" NaN there; "fit_gram", "fit_proj" and "fit_status" keep the bits
        of the unconstrained fit; the sky arrays with sky_order only, "fit_chi2" and "fit_npix" with weight_fields only - plus
        {"fit_scale_free" (N, bands): the fit_scale of the unconstrained call, bit for bit; "fit_clamped" (N, bands) int32;
        "fit_dual" (N, bands): the multiplier y_i >= 0 of a clamped galaxy, +0.0 of a passive one, NaN with FIT_INELIGIBLE or
        FIT_DROPPED; per field "nonneg_iters" (M, bands) int32: the factorisations (1: the unconstrained fit was feasible and
        every shared array has its bits; 0: no unknowns), "nonneg_status" (M, bands) int32: 0 converged, 1 max_iter reached -
        the rows then hold the last iterate and may be negative}."""
        stamps, places, data, fp = _fit_scene_inputs(stamps, places, data_fields, field_ptr)
        n, cs, nb, M = stamps.shape[0], stamps.shape[1], stamps.shape[3], data.shape[0]
        sky, order, sky_ptrs = _fit_sky_args(sky_order, M, nb)
        par = fit_flux_params(min_pivot, scratch_bytes)
        max_iter = nonneg_max_iter(max_iter)
        weights = None if weight_fields is None else check_fit_weights(weight_fields, data.shape)
        out, ptrs = _fit_flux_out(n, nb, weights is not None)
        if weights is None:
            ptrs += [None, None]
        out.update(sky)
        nn, nn_ptrs = _fit_nonneg_out(n, M, nb)
        out.update(nn)
        if M:
            check(lib.dv_scene_fit_flux_nonneg(self._h, _fp(stamps), _ip(places), fp.ctypes.data_as(C.POINTER(C.c_int64)), n, cs,
                                               nb, _dp(data), None if weights is None else _dp(weights), M, data.shape[1],
                                               C.byref(par), order, max_iter, *ptrs, *sky_ptrs, *nn_ptrs))
        return out

    def scene_fit_flux_sky_gram(self, stamps, places, data_field, sky_order: int = 0, weight_field=None) -> Dict[str, np.ndarray]:
        """Step 1 of scene_fit_flux_sky for one field (dv_scene_fit_flux_sky_gram): returns {"gram" (bands, n + q, n + q): the
        lower triangle of the bordered matrix [[G, E], [E^T, K]], 0.0 above the diagonal; "rhs" (n + q, bands): h, then c}
        with the bits the fit works on.  The arguments are scene_fit_flux_gram's; weight_field (F, F, bands) or None."""
        stamps = np.ascontiguousarray(stamps, dtype=np.float32)
        if stamps.ndim != 4 or stamps.shape[1] != stamps.shape[2]:
            raise ValueError(f"expected square stamps (n, cs, cs, bands), got {stamps.shape}")
        n, cs, nb = stamps.shape[0], stamps.shape[1], stamps.shape[3]
        data = np.ascontiguousarray(data_field, dtype=np.float64)
        if data.ndim != 3 or data.shape[0] != data.shape[1] or data.shape[2] != nb:
            raise ValueError(f"expected one data field (F, F, {nb}), got {data.shape}")
        places = _i32_rows(places, "stamp placements") if n else np.zeros((0, 2), np.int32)
        if places.shape != (n, 2):
            raise ValueError(f"expected places ({n}, 2), got {places.shape}")
        if n > FIT_FLUX_MAX_N:
            raise ValueError(f"{n} galaxies in one field, the dense flux fit takes at most {FIT_FLUX_MAX_N}")
        nt = n + sky_terms(sky_order)
        weights = None if weight_field is None else check_fit_weights(weight_field, (1,) + data.shape)
        out = dict(gram=np.zeros((nb, nt, nt), np.float64), rhs=np.zeros((nt, nb), np.float64))
        check(lib.dv_scene_fit_flux_sky_gram(self._h, _fp(stamps), _ip(places), n, cs, nb, _dp(data),
                                             None if weights is None else _dp(weights), data.shape[0], int(sky_order),
                                             _dp(out["gram"]), _dp(out["rhs"])))
        return out

    CATALOG_KEYS = CATALOG_KEYS

    def scene_detect(self, fields_r, thresh: float = 1.5, minarea: int = 4, nthresh: int = 64, cont: float = 1e-5,
                     filter_kernel=None, back_size: int = 64, back_filter: int = 3, return_maps: bool = False,
                     workspace_bytes: int = 0, weights=None, mask=None, noise=None,
                     filter_type: str = "conv") -> Dict[str, np.ndarray]:
        """Source detection on one band of M fields (detect/detection.py's sep call, on the GPU).

        fields_r (M, H, W).  SExtractor's method, float64: background meshes of back_size px with a back_filter median
        filter, D = the background-subtracted field correlated with filter_kernel / sum|k| (None: the 7 x 7
        pixel-integrated Gaussian), components of D > thresh * globalrms with >= minarea pixels, nthresh-level
        deblending with contrast cont.  Returns the catalog {field, parent, npix, peak, flux, x (column), y (row)}, one row
        per object ordered by field, component and peak pixel, plus offsets (M + 1: the rows of field f are
        offsets[f]:offsets[f + 1]) and globalrms (M,); with return_maps also back, rms, D (M, H, W) and labels (M, H, W)
        (the component's parent, -1 outside kept components).  workspace_bytes caps the device workspace per launch
        (0: 4 GiB); a field that needs more is refused.

        weights and / or mask: detection with a per-pixel noise map and a mask (dv_scene_detect_weighted, DESIGN.md
        section 7z).  weights (M, H, W): a pixel counts iff 0 < w < inf; mask (M, H, W) booleans, True = bad, zeroes the
        weights; a mask alone means unit weights and noise="relative".  noise="absolute" (the default with weights): w is
        an inverse variance and thresh is in units of the pixel's own sigma; noise="relative": w is a relative weight and
        the threshold is thresh * globalrms.  filter_type "conv": S = (sum kn v) sqrt(w); "matched":
        S = (sum kn v w) / sqrt(sum kn^2 w).  The D map then holds S and peak is its maximum; the fields must be finite only
        at counting pixels; the result gains bad_meshes (M,), the meshes of every field with fewer than half of their
        pixels counting; a field without a good mesh has no objects, globalrms NaN and labels -1.  With weights and mask
        both None the call is the unweighted one, argument for argument (noise and filter_type must then be left alone)."""
        weighted = weights is not None or mask is not None
        wts = None
        if weighted:
            shape = np.shape(fields_r)
            if len(shape) != 3:
                raise ValueError(f"expected fields (M, H, W), got {shape}")
            wts, noise_id, filter_id = check_detect_weights(shape, weights, mask, noise, filter_type, thresh)
        elif noise is not None or filter_type != "conv":
            raise ValueError("noise and filter_type belong to the weighted call: give weights, a mask or both")
        f = check_detect_args(fields_r, thresh, minarea, nthresh, cont, filter_kernel, back_size, back_filter,
                              workspace_bytes, weights=wts)
        M, H, W = f.shape
        params, kern = _detect_params(thresh, cont, minarea, nthresh, back_size, back_filter, filter_kernel, workspace_bytes)
        maps = {}
        if return_maps:
            maps = dict(back=np.empty((M, H, W)), rms=np.empty((M, H, W)), D=np.empty((M, H, W)),
                        labels=np.empty((M, H, W), np.int32))
        if weighted:
            bad = np.zeros(M, np.int32)
            wstruct = _lib.DvDetectWeights(_dp(wts), noise_id, filter_id)

        def call(cap, n, offsets, grms, columns):
            args = [self._h, _dp(f), M, H, W, C.byref(params), cap, n, offsets, grms, *columns,
                    _dp(maps.get("back")), _dp(maps.get("rms")), _dp(maps.get("D")),
                    _ip(maps["labels"]) if return_maps else None]
            if weighted:
                check(lib.dv_scene_detect_weighted(*args, C.byref(wstruct), _ip(bad)))
            else:
                check(lib.dv_scene_detect(*args))

        out, _ = _run_detect(M, H * W, call)
        out.update(maps)
        if weighted:
            out["bad_meshes"] = bad
        return out

    def scene_detect_multiband(self, fields, bands=None, band_weights=None, thresh: float = 1.5, minarea: int = 4,
                               nthresh: int = 64, cont: float = 1e-5, filter_kernel=None, back_size: int = 64,
                               back_filter: int = 3, return_maps: bool = False, workspace_bytes: int = 0, weights=None,
                               mask=None, noise=None, filter_type: str = "conv") -> Dict[str, np.ndarray]:
        """Source detection on the inverse-variance weighted combination of several bands (dv_scene_detect_multiband,
        DESIGN.md section 7za).

        fields (M, H, W, nb), interleaved as the network reads them.  bands: k distinct band numbers (None: all), their order
        is the order of every sum; band_weights c_j > 0 (None: all 1.0): the spectral shape the combination is matched to.
        Per selected band the background of scene_detect gives back_j, rms_j and v_j = data_j - back_j; the band's weight
        is w_j = 1 / rms_j^2, with weights (M, H, W, k) P_j / rms_j^2 (noise="relative") or P_j (noise="absolute", the
        default with weights); mask (M, H, W) or (M, H, W, k), True = bad, zeroes the planes, and a mask alone means unit
        planes and noise="relative".  A band counts at a pixel iff 0 < w_j < inf (with planes also 0 < P_j < inf).
        V = sum c_j w_j v_j / sum c_j^2 w_j over the counting bands, Wt = sum c_j^2 w_j its inverse variance; segmentation,
        deblending and the catalogue run on them as in scene_detect(weights=Wt, noise="absolute"): thresh (> 0) is in units
        of the combined pixel's own sigma, D holds the significance, flux and the barycentres are sums over V.  The fields
        must be finite in every selected band where that band counts (everywhere without planes).

        Returns the dictionary of scene_detect plus band_globalrms (M, k) and bad_meshes (M, k); globalrms (M,) is
        1 / sqrt(sum c_j^2 / globalrms_j^2), a diagnostic.  With return_maps also back, rms (M, H, W, k) and V, Wt, D, labels
        (M, H, W)."""
        f = np.ascontiguousarray(fields, dtype=np.float64)
        if f.ndim != 4 or min(f.shape[1:]) < 1:
            raise ValueError(f"expected fields (M, H, W, bands), got {f.shape}")
        M, H, W, nb = f.shape
        sel, cw = check_detect_bands(nb, bands, band_weights)
        k = len(sel)
        planes, noise_id, filter_id = check_detect_band_planes((M, H, W, k), weights, mask, noise, filter_type, thresh)
        _check_multiband_finite(f, sel, planes)
        check_detect_args(np.zeros((0, H, W)), thresh, minarea, nthresh, cont, filter_kernel, back_size, back_filter,
                          workspace_bytes)
        params, kern = _detect_params(thresh, cont, minarea, nthresh, back_size, back_filter, filter_kernel, workspace_bytes)
        bgrms = np.zeros((M, k), np.float64)
        bad = np.zeros((M, k), np.int32)
        maps = {}
        if return_maps:
            maps = dict(back=np.empty((M, H, W, k)), rms=np.empty((M, H, W, k)), V=np.empty((M, H, W)), Wt=np.empty((M, H, W)),
                        D=np.empty((M, H, W)), labels=np.empty((M, H, W), np.int32))
        bstruct = _lib.DvDetectBands(_ip(sel), k, _dp(cw), _dp(planes), noise_id, filter_id)

        def call(cap, n, offsets, grms, columns):
            check(lib.dv_scene_detect_multiband(
                self._h, _dp(f), M, H, W, nb, C.byref(params), cap, n, offsets, grms, *columns,
                *[_dp(maps.get(key)) for key in ("back", "rms", "V", "Wt", "D")],
                _ip(maps["labels"]) if return_maps else None, C.byref(bstruct), _dp(bgrms), _ip(bad)))

        out, _ = _run_detect(M, H * W, call)
        out.update(band_globalrms=bgrms, bad_meshes=bad, **maps)
        return out

    def scene_detect_objects(self, fields, bands=None, band_weights=None, thresh: float = 1.5, minarea: int = 4,
                             nthresh: int = 64, cont: float = 1e-5, filter_kernel=None, back_size: int = 64,
                             back_filter: int = 3, workspace_bytes: int = 0, weights=None, mask=None, noise=None,
                             filter_type: str = "conv", segmentation_map: bool = False,
                             columns: bool = True) -> Dict[str, np.ndarray]:
        """The detector with the object segmentation map and the isophotal shapes (dv_scene_detect_objects, DESIGN.md
        section 7zb).

        fields (M, H, W): scene_detect, argument for argument (weights / mask: its weighted call); fields (M, H, W, nb):
        scene_detect_multiband with bands, band_weights and the planes in weights / mask.  Returns the dictionary of that call
        (without maps) plus, per object over the pixels the deblender gave it: the inclusive box xmin, xmax, ymin, ymax;
        xpeak, ypeak, the pixel of peak; vpeak at xvpeak, yvpeak, the largest background-subtracted value; dflux, the sum of
        the thresholded map D; x_iso, y_iso and x2, y2, xy, the first and second moments with weights D (SExtractor's
        singular rule applied); flag, bits 1 blended, 2 at the border, 4 singular rule applied, 8 next to a pixel that does
        not count; the derived a, b, theta, cxx, cyy, cxy; and with segmentation_map segmap (M, H, W) int32: 0 outside
        every object, k + 1 on the pixels of row offsets[f] + k of field f.  columns=False leaves the columns out (the
        segmap alone).  thresh must be >= 0."""
        return _scene_detect_objects(self, fields, bands, band_weights, thresh, minarea, nthresh, cont, filter_kernel, back_size,
                                     back_filter, workspace_bytes, weights, mask, noise, filter_type, segmentation_map,
                                     columns, None)

    def scene_detect_clean(self, fields, bands=None, band_weights=None, thresh: float = 1.5, minarea: int = 4,
                           nthresh: int = 64, cont: float = 1e-5, filter_kernel=None, back_size: int = 64,
                           back_filter: int = 3, workspace_bytes: int = 0, weights=None, mask=None, noise=None,
                           filter_type: str = "conv", segmentation_map: bool = False, columns: bool = True,
                           clean_param: float = 1.0) -> Dict[str, np.ndarray]:
        """scene_detect_objects followed by SExtractor's cleaning pass (dv_scene_detect_clean; sep's
        clean=True, which the reference's sep call leaves on): an object that would not have been detected without the
        extrapolated Moffat wings of a brighter neighbour of its field is merged into that neighbour.  clean_param is the
        profile's beta (> 0; larger: steeper wings, less is absorbed).

        Arguments as in scene_detect_objects; thresh must be > 0 and minarea <= 64.  Returns its dictionary over the cleaned
        rows - a merged row has npix, flux and dflux summed, the peak and vpeak of its brightest member, the union of the
        boxes, the OR of the flags with bit 16, and the survivor's own x, y, x_iso, y_iso, x2, y2, xy and parent - plus
        nmerged (1 + the objects merged into the row), mthresh (the minarea-th largest D - T of the row's own pixels) and
        n_raw (M,), the objects of every field before the pass.  segmap carries the cleaned rows' numbers.  columns=False
        leaves the object columns out (the catalogue, nmerged, mthresh and n_raw alone, with or without the segmap).  A
        field in which nothing is absorbed has the bits of scene_detect_objects."""
        check_detect_clean(clean_param, thresh, minarea)
        return _scene_detect_objects(self, fields, bands, band_weights, thresh, minarea, nthresh, cont, filter_kernel, back_size,
                                     back_filter, workspace_bytes, weights, mask, noise, filter_type, segmentation_map,
                                     columns, float(clean_param))

    def close(self):
        """Destroys the engines created on this context, then the context.  Idempotent."""
        for eng in list(self._engines):
            eng.close()
        if self._h:
            lib.dv_ctx_destroy(self._h)
            self._h = C.c_void_p()
        if self.group is not None and self._owns_group:
            try:
                self.group.close()
            except Exception:
                pass
        self.group = None
        Context._live.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@atexit.register
def _close_all_contexts():
    global _default_ctx
    for ctx in list(Context._live):
        try:
            ctx.close()
        except Exception:
            pass
    _default_ctx = None


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0, 0, 1, None)
    return _default_ctx


def set_default_context(ctx: Optional[Context]):
    global _default_ctx
    _default_ctx = ctx


class Engine:
    """Weights, Adam state, workspaces and step functions of one conv-VAE on one GPU."""

    def __init__(self, cfg: DvConfig, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.cfg = cfg
        self._h = C.c_void_p()
        if not self.ctx._h:
            raise RuntimeError("the Context of this Engine has been closed")
        check(lib.dv_model_create(self.ctx._h, C.byref(cfg), C.byref(self._h)))
        self.ctx._engines.add(self)
        self.specs = arch_specs(cfg)
        self.index = {n: i for i, (n, _, _) in enumerate(self.specs)}
        self.latent = cfg.latent_dim
        self.tw = self.latent + self.latent * (self.latent + 1) // 2
        self.stamp_shape = (cfg.height, cfg.width, cfg.bands)
        self.max_batch = cfg.max_batch
        self._streamed = {}            # slot -> (x, y) host arrays a streamed slot reads (kept alive here)
        self._field_sets = weakref.WeakSet()    # resident field sets opened on this engine (the library frees them with it)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if self._h:
            for fs in list(self._field_sets):
                fs._h = C.c_void_p()           # dv_model_destroy frees the sets: their handles die with the model
            lib.dv_model_destroy(self._h)
            self._h = C.c_void_p()
        try:
            self.ctx._engines.discard(self)
        except Exception:
            pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters -------------------------------------------------------------------------
    def init(self, seed: int = 0):
        check(lib.dv_model_init(self._h, seed))

    def _tensor(self, fn, i, *extra) -> np.ndarray:
        name, shape, _ = self.specs[i]
        a = np.empty(shape, dtype=np.float32)
        check(fn(self._h, i, *extra, _fp(a), a.nbytes))
        return a

    def get_param(self, key) -> np.ndarray:
        return self._tensor(lib.dv_model_get_param, self._idx(key))

    def get_grad(self, key) -> np.ndarray:
        return self._tensor(lib.dv_model_get_grad, self._idx(key))

    def get_slot(self, key, which: int) -> np.ndarray:
        return self._tensor(lib.dv_model_get_slot, self._idx(key), which)

    def set_param(self, key, value):
        i = self._idx(key)
        a = _f32c(value, self.specs[i][1])
        check(lib.dv_model_set_param(self._h, i, _fp(a), a.nbytes))

    def set_slot(self, key, which: int, value):
        i = self._idx(key)
        a = _f32c(value, self.specs[i][1])
        check(lib.dv_model_set_slot(self._h, i, which, _fp(a), a.nbytes))

    def _idx(self, key) -> int:
        return key if isinstance(key, int) else self.index[key]

    def get_params(self) -> Dict[str, np.ndarray]:
        return {n: self.get_param(i) for i, (n, _, _) in enumerate(self.specs)}

    def set_params(self, params: Dict[str, np.ndarray]):
        for n, v in params.items():
            self.set_param(n, v)

    def set_trainable(self, encoder: bool, decoder: bool):
        check(lib.dv_model_set_trainable(self._h, int(encoder), int(decoder)))

    def optimizer_reset(self, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-7):
        check(lib.dv_optimizer_reset(self._h, lr, beta1, beta2, eps))

    @property
    def iterations(self) -> int:
        it = C.c_int64()
        check(lib.dv_optimizer_get_iter(self._h, C.byref(it)))
        return it.value

    @iterations.setter
    def iterations(self, v: int):
        check(lib.dv_optimizer_set_iter(self._h, int(v)))

    # -- data -------------------------------------------------------------------------------
    def upload(self, slot: int, x, y):
        x = _f32c(x)
        y = _f32c(y)
        if x.shape != y.shape or x.shape[1:] != self.stamp_shape:
            raise ValueError(f"expected x, y of shape (N,{self.stamp_shape}), got {x.shape} and {y.shape}")
        check(lib.dv_data_upload(self._h, slot, _fp(x), _fp(y), x.shape[0]))
        self._streamed.pop(slot, None)
        return x.shape[0]

    def open_stream(self, slot: int, x, y):
        """Slot `slot` reads its rows from the host arrays x, y on every step (dv_data_stream_open) instead of holding
        them in HBM: the step functions then name rows of x / y, which are gathered (float64 cast to float32) and copied
        to the device step by step.  x, y: float32 or float64 arrays of shape (N, H, W, C) - np.memmap included - whose
        rows are each contiguous; their own buffers are used, never a copy.  The engine keeps references to them until
        the slot is freed, uploaded or reopened; their contents must not change meanwhile."""
        arrs = []
        for a, what in ((x, "x"), (y, "y")):
            if not isinstance(a, np.ndarray):
                raise TypeError(f"{what}: open_stream reads a numpy array's own buffer, got {type(a).__name__}")
            if a.dtype not in (np.float32, np.float64) or not a.dtype.isnative:
                raise ValueError(f"{what}: a streamed slot reads native float32 or float64 rows, got {a.dtype}")
            if a.ndim != 4 or a.shape[1:] != self.stamp_shape:
                raise ValueError(f"{what}: expected shape (N,{self.stamp_shape}), got {a.shape}")
            row = np.empty(a.shape[1:], a.dtype)
            if a.shape[0] and (a.strides[1:] != row.strides):
                raise ValueError(f"{what}: every row of a streamed array must be contiguous (strides {a.strides})")
            arrs.append(a)
        x, y = arrs
        if x.shape[0] != y.shape[0]:
            raise ValueError(f"x has {x.shape[0]} rows, y {y.shape[0]}")
        check(lib.dv_data_stream_open(self._h, slot, C.c_void_p(x.ctypes.data), int(x.dtype == np.float64),
                                      C.c_void_p(y.ctypes.data), int(y.dtype == np.float64), x.shape[0],
                                      x.strides[0], y.strides[0]))
        self._streamed[slot] = (x, y)
        return x.shape[0]

    def data_info(self, slot: int) -> Dict[str, int]:
        """mode (0 empty, 1 resident, 2 streamed), rows, and the bytes the slot has moved host -> device since it was
        uploaded or opened."""
        mode, n, h2d = C.c_int32(), C.c_int64(), C.c_int64()
        check(lib.dv_data_info(self._h, slot, C.byref(mode), C.byref(n), C.byref(h2d)))
        return {"mode": mode.value, "n": n.value, "h2d_bytes": h2d.value}

    def free_data(self, slot: int):
        check(lib.dv_data_free(self._h, slot))
        self._streamed.pop(slot, None)

    # -- steps ------------------------------------------------------------------------------
    def _step(self, fn, slot, idx, first, B, global_batch, eps, seed) -> Dict[str, float]:
        out = np.zeros(_lib.DV_N_SCALARS, dtype=np.float32)
        ip = None
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            B = idx.size
            ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
        if eps is not None:
            eps = _f32c(eps, (B, self.latent))
        check(fn(self._h, slot, ip, int(first), int(B), int(global_batch or 0), _fp(eps), int(seed), _fp(out)))
        return {k: float(out[i]) for i, k in enumerate(_lib.SCALAR_NAMES)}

    def train_step(self, slot=0, idx=None, first=0, B=None, global_batch=None, eps=None, seed=0):
        return self._step(lib.dv_train_step, slot, idx, first, B, global_batch, eps, seed)

    def eval_step(self, slot=1, idx=None, first=0, B=None, global_batch=None, eps=None, seed=0):
        return self._step(lib.dv_eval_step, slot, idx, first, B, global_batch, eps, seed)

    def grad_step(self, slot=0, idx=None, first=0, B=None, global_batch=None, eps=None, seed=0):
        return self._step(lib.dv_grad_step, slot, idx, first, B, global_batch, eps, seed)

    def train_step_async(self, ticket, slot=0, idx=None, first=0, B=None, global_batch=None, seed=0):
        """Queues a training step under `ticket` (0..3); step_result(ticket) returns its scalars later."""
        ip = None
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            B = idx.size
            ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
        check(lib.dv_train_step_async(self._h, slot, ip, int(first), int(B), int(global_batch or 0), int(seed), int(ticket)))

    def step_result(self, ticket) -> Dict[str, float]:
        out = np.zeros(_lib.DV_N_SCALARS, dtype=np.float32)
        check(lib.dv_step_result(self._h, int(ticket), _fp(out)))
        return {k: float(out[i]) for i, k in enumerate(_lib.SCALAR_NAMES)}

    def train_steps(self, slot, first, B, steps, global_batch=None, seed=0) -> Dict[str, float]:
        out = np.zeros(_lib.DV_N_SCALARS, dtype=np.float32)
        check(lib.dv_train_steps(self._h, slot, int(first), int(B), int(global_batch or 0), int(steps), int(seed),
                                 _fp(out)))
        return {k: float(out[i]) for i, k in enumerate(_lib.SCALAR_NAMES)}

    # -- inference --------------------------------------------------------------------------
    def set_normalise(self, on: bool):
        """tanh(arcsinh) on inference inputs and the inverse on the predicted mean, on the GPU (deblend(normalise=True))."""
        check(lib.dv_model_set_normalise(self._h, 1 if on else 0))

    def set_mse_sample(self, on: bool):
        """The "mse" scalar of the step functions against a SAMPLE of the output distribution (Keras semantics of the
        reference's compile(metrics=["mse"]), model.py:158) instead of its mean."""
        check(lib.dv_model_set_mse_sample(self._h, 1 if on else 0))

    def keep_outputs(self, on: bool):
        """Gradient / train steps also write loc and scale of their forward pass (activation("loc"), activation("scale"));
        off by default - a train step has no reader for them."""
        check(lib.dv_model_set_keep_outputs(self._h, 1 if on else 0))

    def _infer_bufs(self, N, want, out=None):
        """The float32 result arrays of an N-stamp inference call in the C-ABI's order (loc, scale, mu, zstd, z), None for
        what is not in `want`: the caller's own out[k] (reused across calls) where given, otherwise from the host pool."""
        bufs = {}
        for k in ("loc", "scale", "mu", "zstd", "z"):
            shape = (N,) + self.stamp_shape if k in ("loc", "scale") else (N, self.latent)
            if k not in want:
                bufs[k] = None
            elif out is not None and k in out:
                if out[k].shape != shape or out[k].dtype != np.float32 or not out[k].flags.c_contiguous:
                    raise ValueError(f"out[{k!r}] must be a C-contiguous float32 array of shape {shape}")
                bufs[k] = out[k]
            else:
                bufs[k] = _host_pool.empty(shape, np.float32)
        return bufs

    def infer(self, x, eps=None, seed=0, want=("loc", "scale"), out=None) -> Dict[str, np.ndarray]:
        """One stochastic forward pass over all stamps.  float64 arrays (numpy's default, what the reference's callers
        pass) go to the engine as they are: the float32 cast of deblender.py:18 happens while the library stages them."""
        x = np.asarray(x)
        f64 = x.dtype == np.float64 and x.flags.c_contiguous
        if not f64:
            x = _f32c(x)
        if x.ndim != 4 or x.shape[1:] != self.stamp_shape:
            raise ValueError(f"expected images of shape (N,{self.stamp_shape}), got {x.shape}")
        N = x.shape[0]
        bufs = self._infer_bufs(N, want, out)
        if eps is not None:
            eps = _f32c(eps, (N, self.latent))
        if f64:
            check(lib.dv_infer_f64(self._h, _dp(x), N, _fp(eps), int(seed), *map(_fp, bufs.values())))
        else:
            check(lib.dv_infer(self._h, _fp(x), N, _fp(eps), int(seed), *map(_fp, bufs.values())))
        return {k: v for k, v in bufs.items() if v is not None}

    # -- cutouts of fields that sit on the GPU (DESIGN.md sections 7, 7f) --------------------------
    @staticmethod
    def _field_args(fields, starts, field_ptr, places=None):
        """The checked inputs of the many-field calls: the float64 fields (M, F, F, bands), the number of stamps, and the
        C-ABI's arguments from `fields` to `N` (with `places` before field_ptr where the call takes them)."""
        fields = _check_fields(fields)
        starts = _i32_rows(starts, "cutout starts")
        if places is not None:
            places = _i32_rows(places, "stamp placements")
            if places.shape != starts.shape:
                raise ValueError(f"{starts.shape[0]} cutout starts but {places.shape[0]} placements")
        N = starts.shape[0]
        fp = check_field_ptr(field_ptr, fields.shape[0], N)
        args = [_dp(fields), fields.shape[0], fields.shape[1], fields.shape[3], _ip(starts)]
        if places is not None:
            args.append(_ip(places))
        return fields, N, args + [fp.ctypes.data_as(C.POINTER(C.c_int64)), N]

    @staticmethod
    def _composite_out(shape, N, residual, mse_center, epistemic=False):
        """The result dictionary of the composite calls - float64 fields of `shape`, per-stamp scalars (N,) - and its
        pointers in the C-ABI's order, None for what is not wanted."""
        out = {"mean_fields": np.empty(shape, np.float64), "stddev_fields": np.empty(shape, np.float64)}
        if epistemic:
            out["epistemic_fields"] = np.empty(shape, np.float64)
        if residual:
            out["residual_fields"] = np.empty(shape, np.float64)
        if mse_center:
            out["mse_center"] = np.empty((N,), np.float64)
        if epistemic:
            out["eps_norm"] = np.empty((N,), np.float64)
        keys = ["mean_fields", "stddev_fields", "residual_fields", "mse_center"]
        if epistemic:
            keys = keys[:2] + ["epistemic_fields"] + keys[2:] + ["eps_norm"]
        return out, [_dp(out.get(k)) for k in keys]

    def infer_fields(self, fields, starts, field_ptr, seed=0, want=("loc", "scale"), out=None) -> Dict[str, np.ndarray]:
        """infer() on the cutouts fields[m, x:x+H, y:y+H, :] of M float64 fields (M, F, F, bands), gathered and cast on the
        GPU in one engine call (dv_infer_fields): rows field_ptr[m]:field_ptr[m + 1] of `starts` are windows (x, y) of field
        m.  The N stamps of all fields form one list that runs through the network in full chunks, whatever field a stamp
        belongs to; stamp i draws noise row i, and no stamp visits the host.  Bit-identical to infer() on the concatenated
        cutouts with the same seed."""
        fields, N, args = Engine._field_args(fields, starts, field_ptr)
        bufs = self._infer_bufs(N, want, out)
        check(lib.dv_infer_fields(self._h, *args, int(seed), *map(_fp, bufs.values())))
        return {k: v for k, v in bufs.items() if v is not None}

    def infer_fields_keep(self, fields, starts, field_ptr, seed=0, want=("loc", "scale")) -> Dict[str, np.ndarray]:
        """infer_fields() for a caller that also needs the float64 cutouts (dv_infer_fields_keep): the wanted outputs plus
        "cutouts" (N,) + stamp shape, assembled on the host from the fields while the GPU runs the forward passes -
        bit-identical to ctx.scene_extract(field, starts, H) field by field."""
        fields, N, args = Engine._field_args(fields, starts, field_ptr)
        bufs = self._infer_bufs(N, want)
        cut = _host_pool.empty((N,) + self.stamp_shape, np.float64)
        check(lib.dv_infer_fields_keep(self._h, *args, int(seed), *map(_fp, bufs.values()), _dp(cut)))
        res = {k: v for k, v in bufs.items() if v is not None}
        res["cutouts"] = cut
        return res

    def infer_fields_composite(self, fields, starts, places, field_ptr, seed=0, residual=True,
                               mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields() with the compositing that follows it in the reference done on the GPU
        (dv_infer_fields_composite): returns {"mean_fields", "stddev_fields", ["residual_fields"]} (M, F, F, bands) and
        ["mse_center"] (N,) - float64 sums of the network's mean / stddev stamps placed at `places` (row, col of each
        stamp's top-left corner; off-field parts are dropped), the fields minus the mean stamps, and each stamp's
        centre-10x10 MSE against its cutout.  A field's results are the sums of its own stamps in object order, the same
        bits whatever other fields the call holds; a field without stamps gets zeros and its residual is the field."""
        fields, N, args = Engine._field_args(fields, starts, field_ptr, places)
        out, ptrs = Engine._composite_out(fields.shape, N, residual, mse_center)
        check(lib.dv_infer_fields_composite(self._h, *args, int(seed), *ptrs))
        return out

    @staticmethod
    def _measure_places(places, return_fields, always=None):
        """The placements an infer_fields_measure* call passes on: None in the catalogue-only form, unless its extra composites
        on the device all the same - `always` is then what to say when they are missing."""
        if places is None and (always or return_fields):
            raise ValueError(always or "places are needed to composite the fields; return_fields=False measures without them")
        return places if always or return_fields else None

    def _fields_measure(self, fn, fields, starts, field_ptr, places, seed, measure, return_fields, residual, mse_center,
                        extras=None, between=()):
        """The body the infer_fields_measure* methods share.  fn: the C call; places: what _measure_places gave; measure:
        (band, sigma0, tol, max_iter); between: what the call takes between seed and params; extras(N, bands): the call's
        own results in the order of the C ABI, each a pair (dictionary, arguments) - the arguments are what the call takes
        for it after the catalogue's, parameters first.  Every check comes before the first use of self."""
        fields, N, args = Engine._field_args(fields, starts, field_ptr, places)
        nb = fields.shape[3]
        par = measure_params(*measure, nb)
        extras = extras(N, nb) if extras else []
        if return_fields:
            out, ptrs = Engine._composite_out(fields.shape, N, residual, mse_center)
        else:
            out = {"mse_center": np.empty((N,), np.float64)} if mse_center else {}
            ptrs = [None, None, None, _dp(out.get("mse_center"))]
        if places is None:
            args = args[:5] + [None] + args[5:]
        out.update(flux=np.zeros((N, nb), np.float64), flux_err=np.zeros((N, nb), np.float64),
                   shape=np.zeros((N, 5), np.float64), iters=np.zeros(N, np.int32), status=np.zeros(N, np.int32))
        ptrs += [_dp(out["flux"]), _dp(out["flux_err"]), _dp(out["shape"]), _ip(out["iters"]), _ip(out["status"])]
        for res, res_args in extras:
            out.update(res)
            ptrs += res_args
        check(fn(self._h, *args, int(seed), *between, C.byref(par), *ptrs))
        return out

    def infer_fields_measure(self, fields, starts, field_ptr, places=None, seed=0, band: int = 2, sigma0: float = 3.0,
                             tol: float = 1e-10, max_iter: int = 200, return_fields=True, residual=True,
                             mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_composite() with the catalogue measurement of scene_measure as one more stage of the pipeline
        (dv_infer_fields_measure): behind every chunk's forward pass the chunk's mean and stddev stamps
        are measured where they lie in device memory.  Returns infer_fields_composite's dictionary plus {"flux", "flux_err"
        (N, bands), "shape" (N, 5), "iters", "status" (N,)} - rows are the global stamp numbers, the bits those of
        scene_measure on the stamps infer_fields returns for the same seed.  return_fields=False is the catalogue-only
        call: no field is composited, allocated or downloaded, `places` is not needed, and the dictionary holds the
        catalogue (and mse_center) only."""
        places = Engine._measure_places(places, return_fields)
        return Engine._fields_measure(self, lib.dv_infer_fields_measure, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center)

    def infer_cutouts_measure(self, field, starts, places=None, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure() for one field (F, F, bands): the field-sized results under singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure(fields, starts, fp, places=places, seed=seed, **kw))

    def scene_measure(self, mean, stddev=None, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_measure on this engine's GPU context."""
        return self.ctx.scene_measure(mean, stddev, **kw)

    def infer_fields_measure_blend(self, fields, starts, field_ptr, places, seed=0, band: int = 2, sigma0: float = 3.0,
                                   tol: float = 1e-10, max_iter: int = 200, return_fields=True, residual=True,
                                   mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure() plus the blendedness sums (dv_infer_fields_measure_blend): returns its
        dictionary, bit for bit, plus scene_blend's {"blend" (N, 4), "npix" (N,)} - the bits of scene_blend on infer_fields'
        mean stamps, infer_fields_measure's rows, infer_fields_composite's mean fields and the source fields as data.  The
        stamp sums run behind every chunk's measurement, the field sums once a field's composite is complete.  `places` is
        always needed: with return_fields=False the mean field is still composited on the device (and never downloaded)."""
        places = Engine._measure_places(places, return_fields, "places are needed for the blendedness sums, with "
                                        "return_fields=False too")

        def extras(N, nb):
            bl = dict(blend=np.zeros((N, 4), np.float64), npix=np.zeros(N, np.int32))
            return [(bl, [_dp(bl["blend"]), _ip(bl["npix"])])]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_blend, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_cutouts_measure_blend(self, field, starts, places, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_blend() for one field (F, F, bands): the field-sized results under singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_blend(fields, starts, fp, places, seed=seed, **kw))

    def scene_blend(self, stamps, shape, status, places, model_fields, data_fields=None, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_blend on this engine's GPU context."""
        return self.ctx.scene_blend(stamps, shape, status, places, model_fields, data_fields, **kw)

    def infer_fields_measure_psf(self, fields, starts, field_ptr, psf, psf_index=None, places=None, seed=0, band: int = 2,
                                 sigma0: float = 3.0, tol: float = 1e-10, max_iter: int = 200, psf_sigma0: float = 2.0,
                                 return_fields=True, residual=True, mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure() plus the PSF-corrected moments (dv_infer_fields_measure_psf): returns
        its dictionary, bit for bit, plus scene_regauss' {"regauss", "regauss_iters", "regauss_status", "psf_shape",
        "psf_aux", "psf_iters", "psf_status"} - the bits of scene_regauss on infer_fields' mean stamps and
        infer_fields_measure's rows.  The PSFs (K, ps, ps) are uploaded and measured once; the correction runs behind every
        chunk's measurement on the stamps in device memory.  psf_index (N,) picks every stamp's PSF (None: PSF 0).
        return_fields=False is the catalogue-only call, as there."""
        places = Engine._measure_places(places, return_fields)

        def extras(N, nb):
            images, index = check_psf_args(psf, psf_index, N, psf_sigma0)
            rg, rg_ptrs = _regauss_out(N, images.shape[0])
            if N == 0:                      # (the library has nothing to run; the PSF rows come from the stamp-level call)
                empty = self.ctx.scene_regauss(np.zeros((0,) + tuple(self.stamp_shape), np.float32), np.zeros((0, 5)),
                                               np.zeros(0, np.int32), images, band=band, psf_sigma0=psf_sigma0, tol=tol,
                                               max_iter=max_iter)
                rg.update({k: empty[k] for k in ("psf_shape", "psf_aux", "psf_iters", "psf_status")})
            return [(rg, [_dp(images), images.shape[0], images.shape[1], _ip(index), float(psf_sigma0)] + rg_ptrs)]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_psf, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_cutouts_measure_psf(self, field, starts, psf, psf_index=None, places=None, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_psf() for one field (F, F, bands): the field-sized results under singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_psf(fields, starts, fp, psf, psf_index, places=places, seed=seed, **kw))

    def scene_regauss(self, stamps, shape, status, psf, psf_index=None, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_regauss on this engine's GPU context."""
        return self.ctx.scene_regauss(stamps, shape, status, psf, psf_index, **kw)

    def infer_fields_measure_aper(self, fields, starts, field_ptr, places=None, seed=0, band: int = 2, sigma0: float = 3.0,
                                  tol: float = 1e-10, max_iter: int = 200, radii=(3.0, 5.0, 8.0), fractions=(0.2, 0.5, 0.8),
                                  subsample: int = 5, kron_factor: float = 2.5, kron_min: float = 3.5, kron_limit: float = 6.0,
                                  bisect_iters: int = 32, return_fields=True, residual=True,
                                  mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure() plus the aperture photometry (dv_infer_fields_measure_aper): returns
        its dictionary, bit for bit, plus scene_aperture's {"ap_flux", "ap_flux_err", "ap_area", "flux_auto",
        "flux_auto_err", "kron", "flux_rho", "aper_flags", "aper_status"} - the bits of scene_aperture on infer_fields' mean
        and stddev stamps and infer_fields_measure's rows.  The photometry runs behind every chunk's measurement on the
        stamps in device memory.  return_fields=False is the catalogue-only call, as there."""
        places = Engine._measure_places(places, return_fields)

        def extras(N, nb):
            apar = aperture_params(radii, fractions, subsample, kron_factor, kron_min, kron_limit, bisect_iters)
            ap, ap_ptrs = _aperture_out(N, nb, apar)
            return [(ap, [C.byref(apar)] + ap_ptrs)]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_aper, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_cutouts_measure_aper(self, field, starts, places=None, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_aper() for one field (F, F, bands): the field-sized results under singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_aper(fields, starts, fp, places=places, seed=seed, **kw))

    def scene_aperture(self, mean, shape, status, stddev=None, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_aperture on this engine's GPU context."""
        return self.ctx.scene_aperture(mean, shape, status, stddev, **kw)

    def infer_fields_measure_aper_data(self, fields, starts, field_ptr, places, seed=0, band: int = 2, sigma0: float = 3.0,
                                       tol: float = 1e-10, max_iter: int = 200, radii=(3.0, 5.0, 8.0),
                                       fractions=(0.2, 0.5, 0.8), subsample: int = 5, kron_factor: float = 2.5,
                                       kron_min: float = 3.5, kron_limit: float = 6.0, bisect_iters: int = 32,
                                       return_fields=True, residual=True, mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure_aper() plus the same apertures on the fields (dv_infer_fields_measure_aper_data, DESIGN.md
        section 7p): returns its dictionary, bit for bit, plus scene_aperture_fields' {"ap_model_sum", "ap_data_sum",
        "ap_field_area", "auto_model_sum", "auto_data_sum", "auto_field_area"} - the bits of scene_aperture_fields on
        infer_fields_measure_aper's rows, infer_fields_composite's mean fields and the source fields as data.  The field sums
        run once a field's composite is complete.  `places` is always needed: with return_fields=False the mean field is still
        composited on the device (and never downloaded)."""
        places = Engine._measure_places(places, return_fields, "places are needed for the apertures on the fields, with "
                                        "return_fields=False too")

        def extras(N, nb):
            apar = aperture_params(radii, fractions, subsample, kron_factor, kron_min, kron_limit, bisect_iters)
            ap, ap_ptrs = _aperture_out(N, nb, apar)
            return [(ap, [C.byref(apar)] + ap_ptrs), _aperture_field_out(N, nb, apar)]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_aper_data, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_cutouts_measure_aper_data(self, field, starts, places, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_aper_data() for one field (F, F, bands): the field-sized results under singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_aper_data(fields, starts, fp, places, seed=seed, **kw))

    def scene_aperture_fields(self, shape, status, places, kron, aper_status, model_fields, data_fields=None,
                              **kw) -> Dict[str, np.ndarray]:
        """Context.scene_aperture_fields on this engine's GPU context."""
        return self.ctx.scene_aperture_fields(shape, status, places, kron, aper_status, model_fields, data_fields, **kw)

    def infer_fields_measure_fit(self, fields, starts, field_ptr, places, seed=0, band: int = 2, sigma0: float = 3.0,
                                 tol: float = 1e-10, max_iter: int = 200, min_pivot: float = 1e-8,
                                 scratch_bytes: int = 256 << 20, return_fields=True, residual=True,
                                 mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure() plus the simultaneous flux fit (dv_infer_fields_measure_fit): returns
        its dictionary, bit for bit, plus scene_fit_flux's {"fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status"} -
        the bits of scene_fit_flux on infer_fields_keep's mean stamps and the source fields.  The mean stamps of every chunk
        are kept on the device and the fit runs once a field's composite is complete.  `places` is always needed, with
        return_fields=False too."""
        places = Engine._measure_places(places, return_fields, "places are needed for the flux fit, with return_fields=False too")

        def extras(N, nb):
            fpar = fit_flux_params(min_pivot, scratch_bytes)
            ff, ff_ptrs = _fit_flux_out(N, nb)
            return [(ff, [C.byref(fpar)] + ff_ptrs)]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_fit, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_cutouts_measure_fit(self, field, starts, places, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_fit() for one field (F, F, bands): the field-sized results under singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_fit(fields, starts, fp, places, seed=seed, **kw))

    def infer_fields_measure_fit_weighted(self, fields, starts, field_ptr, places, weight_fields, seed=0, band: int = 2,
                                          sigma0: float = 3.0, tol: float = 1e-10, max_iter: int = 200, min_pivot: float = 1e-8,
                                          scratch_bytes: int = 256 << 20, return_fields=True, residual=True,
                                          mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure_fit() under per-pixel weights (dv_infer_fields_measure_fit_weighted):
        weight_fields has the shape of fields, the inverse variance of every pixel, 0 (or anything not in (0, inf)) where a
        pixel is masked.  Returns infer_fields_measure's dictionary, bit for bit, plus scene_fit_flux(weight_fields=...)'s
        {"fit_scale", "fit_var", "fit_gram", "fit_proj", "fit_status", "fit_chi2", "fit_npix"} with the bits of that call on
        infer_fields_keep's mean stamps.  The weight fields are resident beside the source fields, group by group."""
        places = Engine._measure_places(places, return_fields, "places are needed for the flux fit, with return_fields=False too")
        fields = _check_fields(fields)
        weights = check_fit_weights(weight_fields, fields.shape)

        def extras(N, nb):
            fpar = fit_flux_params(min_pivot, scratch_bytes)
            ff, ff_ptrs = _fit_flux_out(N, nb, True)
            return [(ff, [C.byref(fpar), _dp(weights)] + ff_ptrs)]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_fit_weighted, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_cutouts_measure_fit_weighted(self, field, starts, places, weight_field, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_fit_weighted() for one field and its weight field (F, F, bands): the field-sized results under
        singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_fit_weighted(fields, starts, fp, places, weight_field, seed=seed, **kw))

    def scene_fit_flux(self, stamps, places, data_fields, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_fit_flux on this engine's GPU context."""
        return self.ctx.scene_fit_flux(stamps, places, data_fields, **kw)

    def infer_fields_measure_fit_groups(self, fields, starts, field_ptr, places, weight_fields=None, seed=0, band: int = 2,
                                        sigma0: float = 3.0, tol: float = 1e-10, max_iter: int = 200, min_pivot: float = 1e-8,
                                        scratch_bytes: int = 256 << 20, return_fields=True, residual=True,
                                        mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure_fit[_weighted]() by blend groups (dv_infer_fields_measure_fit_groups): no
        limit on the galaxies of a field, 1024 per group.  Returns infer_fields_measure's dictionary, bit for bit, plus
        scene_fit_flux_groups' - with "fit_chi2" and "fit_npix" iff weight_fields is given - with the bits of that call on
        infer_fields_keep's mean stamps."""
        places = Engine._measure_places(places, return_fields, "places are needed for the flux fit, with return_fields=False too")
        fields = _check_fields(fields)
        weights = None if weight_fields is None else check_fit_weights(weight_fields, fields.shape)

        def extras(N, nb):
            fpar = fit_flux_params(min_pivot, scratch_bytes)
            ff, ff_ptrs = _fit_flux_out(N, nb, weights is not None)
            if weights is None:
                ff_ptrs += [None, None]
            ff["fit_group"], ff["fit_group_size"] = np.zeros(N, np.int32), np.zeros(N, np.int32)
            return [(ff, [C.byref(fpar), None if weights is None else _dp(weights)] + ff_ptrs +
                     [_ip(ff["fit_group"]), _ip(ff["fit_group_size"])])]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_fit_groups, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_fields_measure_moments_data(self, fields, starts, field_ptr, places, weight_fields=None, seed=0, band: int = 2,
                                          sigma0: float = 3.0, tol: float = 1e-10, max_iter: int = 200, return_fields=True,
                                          residual=True, mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure() plus the adaptive moments on the observed field with the neighbours subtracted
        (dv_infer_fields_measure_moments_data): returns its dictionary, bit for bit, plus
        scene_moments_fields' {"flux_data", "npix_data", "shape_data", "iters_data", "status_data"} - the bits of that call on
        infer_fields_keep's mean stamps, infer_fields_composite's mean fields and the source fields as data, taken once a
        field's composite is complete.  weight_fields has the shape of fields or is None (a mask: a pixel counts iff 0 < W <
        inf).  `places` is always needed: with return_fields=False the mean field is still composited on the device."""
        places = Engine._measure_places(places, return_fields, "places are needed for the moments on the fields, with "
                                        "return_fields=False too")
        fields = _check_fields(fields)
        weights = None if weight_fields is None else check_fit_weights(weight_fields, fields.shape)

        def extras(N, nb):
            md, md_ptrs = _moments_data_out(N, nb)
            return [(md, [None if weights is None else _dp(weights)] + md_ptrs)]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_moments_data, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_cutouts_measure_moments_data(self, field, starts, places, weight_field=None, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_moments_data() for one field and its optional weight field (F, F, bands): the field-sized
        results under singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_moments_data(fields, starts, fp, places, weight_field, seed=seed, **kw))

    def scene_moments_fields(self, stamps, places, model_fields, data_fields, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_moments_fields on this engine's GPU context."""
        return self.ctx.scene_moments_fields(stamps, places, model_fields, data_fields, **kw)

    def scene_fit_flux_groups(self, stamps, places, data_fields, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_fit_flux_groups on this engine's GPU context."""
        return self.ctx.scene_fit_flux_groups(stamps, places, data_fields, **kw)

    def scene_fit_groups(self, places, cutout_size, field_size, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_fit_groups on this engine's GPU context."""
        return self.ctx.scene_fit_groups(places, cutout_size, field_size, **kw)

    def infer_fields_measure_fit_sky(self, fields, starts, field_ptr, places, sky_order: int = 0, weight_fields=None, seed=0,
                                     band: int = 2, sigma0: float = 3.0, tol: float = 1e-10, max_iter: int = 200,
                                     min_pivot: float = 1e-8, scratch_bytes: int = 256 << 20, return_fields=True, residual=True,
                                     mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure_fit[_weighted]() with a sky background fitted jointly (dv_infer_fields_measure_fit_sky,
        DESIGN.md section 7t): sky_order 0 a constant, 1 a plane per field and band; weight_fields None is the unweighted
        fit.  Returns infer_fields_measure's dictionary, bit for bit, plus scene_fit_flux_sky's - the galaxy rows ("fit_chi2"
        and "fit_npix" with weight_fields only) and the per-field "sky_coef", "sky_cov", "sky_status", "sky_npix" - with the
        bits of that call on infer_fields_keep's mean stamps.  Fields without galaxies are solved too."""
        places = Engine._measure_places(places, return_fields, "places are needed for the flux fit, with return_fields=False too")
        fields = _check_fields(fields)
        q = sky_terms(sky_order)
        weights = None if weight_fields is None else check_fit_weights(weight_fields, fields.shape)

        def extras(N, nb):
            fpar = fit_flux_params(min_pivot, scratch_bytes)
            ff, ff_ptrs = _fit_flux_out(N, nb, weights is not None)
            if weights is None:
                ff_ptrs += [None, None]
            sky, sky_ptrs = _fit_sky_out(fields.shape[0], nb, q)
            ff.update(sky)
            return [(ff, [C.byref(fpar), None if weights is None else _dp(weights), int(sky_order)] + ff_ptrs + sky_ptrs)]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_fit_sky, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_cutouts_measure_fit_sky(self, field, starts, places, sky_order: int = 0, weight_field=None, seed=0,
                                      **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_fit_sky() for one field (and its weight field) (F, F, bands): the field-sized results under
        singular key names; the sky arrays keep their leading axis of one field."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_fit_sky(fields, starts, fp, places, sky_order, weight_field, seed=seed,
                                                                  **kw))

    def scene_fit_flux_sky(self, stamps, places, data_fields, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_fit_flux_sky on this engine's GPU context."""
        return self.ctx.scene_fit_flux_sky(stamps, places, data_fields, **kw)

    def infer_fields_measure_fit_nonneg(self, fields, starts, field_ptr, places, sky_order=None, weight_fields=None, seed=0,
                                        band: int = 2, sigma0: float = 3.0, tol: float = 1e-10, max_iter: int = 200,
                                        min_pivot: float = 1e-8, fit_max_iter: int = 100, scratch_bytes: int = 256 << 20,
                                        return_fields=True, residual=True, mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_measure_fit[_weighted / _sky]() with the amplitudes constrained to be >= 0
        (dv_infer_fields_measure_fit_nonneg): sky_order None fits no sky, weight_fields None is the
        unweighted fit, fit_max_iter caps the factorisations per field and band (max_iter is the moments').  Returns
        infer_fields_measure's dictionary, bit for bit, plus scene_fit_flux_nonneg's, with the bits of that call on
        infer_fields_keep's mean stamps."""
        places = Engine._measure_places(places, return_fields, "places are needed for the flux fit, with return_fields=False too")
        fields = _check_fields(fields)
        if sky_order is not None:
            sky_terms(sky_order)
        fit_max_iter = nonneg_max_iter(fit_max_iter)
        weights = None if weight_fields is None else check_fit_weights(weight_fields, fields.shape)

        def extras(N, nb):
            fpar = fit_flux_params(min_pivot, scratch_bytes)
            ff, ff_ptrs = _fit_flux_out(N, nb, weights is not None)
            if weights is None:
                ff_ptrs += [None, None]
            sky, order, sky_ptrs = _fit_sky_args(sky_order, fields.shape[0], nb)
            ff.update(sky)
            nn, nn_ptrs = _fit_nonneg_out(N, fields.shape[0], nb)
            ff.update(nn)
            return [(ff, [C.byref(fpar), None if weights is None else _dp(weights), order, fit_max_iter] + ff_ptrs + sky_ptrs +
                     nn_ptrs)]

        return Engine._fields_measure(self, lib.dv_infer_fields_measure_fit_nonneg, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center, extras)

    def infer_cutouts_measure_fit_nonneg(self, field, starts, places, sky_order=None, weight_field=None, seed=0,
                                         **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_fit_nonneg() for one field (and its weight field) (F, F, bands): the field-sized results under
        singular key names; the per-field arrays keep their leading axis of one field."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_fit_nonneg(fields, starts, fp, places, sky_order, weight_field,
                                                                     seed=seed, **kw))

    def scene_fit_flux_nonneg(self, stamps, places, data_fields, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_fit_flux_nonneg on this engine's GPU context."""
        return self.ctx.scene_fit_flux_nonneg(stamps, places, data_fields, **kw)

    def infer_fields_measure_mc(self, fields, starts, field_ptr, places=None, seed=0, mc_seed=0, nsamples=100, band: int = 2,
                                sigma0: float = 3.0, tol: float = 1e-10, max_iter: int = 200, return_fields=True,
                                residual=True, mse_center=True, keep_samples=False) -> Dict[str, np.ndarray]:
        """infer_fields_measure() plus the Monte-Carlo catalogue (dv_infer_fields_measure_mc): behind
        every chunk's forward pass `nsamples` more stochastic decodes of its encoder output are measured where they lie in
        device memory and folded per galaxy.  Returns infer_fields_measure's dictionary, bit for bit for the same `seed`, plus
        scene_measure_mc's {"flux_mc_mean", "flux_mc_std", "shape_mc_mean", "shape_mc_std", "n_ok"} (and the per-sample rows
        with keep_samples=True) - the bits of scene_measure_mc on the stacked stamps infer_mc(cutouts.astype(float32), 1,
        mc_seed + q)[0].  No epistemic field and no eps_norm are computed; return_fields=False is the catalogue-only call."""
        places = Engine._measure_places(places, return_fields)
        if int(nsamples) < 1:
            raise ValueError(f"nsamples must be at least 1, got {nsamples}")
        return Engine._fields_measure(self, lib.dv_infer_fields_measure_mc, fields, starts, field_ptr, places, seed,
                                      (band, sigma0, tol, max_iter), return_fields, residual, mse_center,
                                      lambda N, nb: [_measure_mc_out(N, nb, int(nsamples), keep_samples)],
                                      between=(int(mc_seed), int(nsamples)))

    def infer_cutouts_measure_mc(self, field, starts, places=None, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_measure_mc() for one field (F, F, bands): the field-sized results under singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_measure_mc(fields, starts, fp, places=places, seed=seed, **kw))

    def scene_measure_mc(self, samples, **kw) -> Dict[str, np.ndarray]:
        """Context.scene_measure_mc on this engine's GPU context."""
        return self.ctx.scene_measure_mc(samples, **kw)

    def open_field_set(self, fields, cumulative=False) -> "FieldSet":
        """Upload M float64 fields (M, F, F, bands) once and keep them, their working and final residuals and the predicted
        sums on the GPU between the passes of an iterative deblending loop (dv_field_set_open)."""
        return FieldSet(self, fields, cumulative)

    # -- the same with the Monte-Carlo epistemic estimate as a pipeline stage --
    @staticmethod
    def _check_mc(nsamples, bands):
        if int(nsamples) < 1:
            raise ValueError(f"nsamples must be at least 1, got {nsamples}")
        if int(bands) < 3:
            raise ValueError(f"the normalised epistemic uncertainty is read from band 2, the fields have {int(bands)} bands")

    def infer_fields_mc_keep(self, fields, starts, field_ptr, seed=0, mc_seed=0, nsamples=100) -> Dict[str, np.ndarray]:
        """infer_fields_keep() plus "epistemic" (N,) + stamp shape, float32: the standard deviation of `nsamples` more
        stochastic decodes of every stamp (dv_infer_fields_mc_keep), run on the GPU behind each chunk's forward pass on the
        encoder output that pass left there.  loc / scale / cutouts are infer_fields_keep's for `seed`, bit for bit;
        "epistemic" is infer_mc(cutouts.astype(float32), nsamples, seed=mc_seed)[1], bit for bit."""
        fields, N, args = Engine._field_args(fields, starts, field_ptr)
        Engine._check_mc(nsamples, fields.shape[3])
        out = {"loc": _host_pool.empty((N,) + self.stamp_shape, np.float32),
               "scale": _host_pool.empty((N,) + self.stamp_shape, np.float32),
               "cutouts": _host_pool.empty((N,) + self.stamp_shape, np.float64),
               "epistemic": _host_pool.empty((N,) + self.stamp_shape, np.float32)}
        check(lib.dv_infer_fields_mc_keep(self._h, *args, int(seed), int(mc_seed), int(nsamples), _fp(out["loc"]),
                                          _fp(out["scale"]), _dp(out["cutouts"]), _fp(out["epistemic"])))
        return out

    def infer_fields_mc_composite(self, fields, starts, places, field_ptr, seed=0, mc_seed=0, nsamples=100, residual=True,
                                  mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_composite() plus "epistemic_fields" (M, F, F, bands) - the Monte-Carlo std stamps of
        infer_fields_mc_keep summed at `places` in float64, object order - and "eps_norm" (N,): sum(std[:, :, 2]) /
        sum(mean[:, :, 2]) per stamp in float64 (dv_infer_fields_mc_composite).  No stamp visits the host; the other
        results are infer_fields_composite's for `seed`, bit for bit."""
        fields, N, args = Engine._field_args(fields, starts, field_ptr, places)
        Engine._check_mc(nsamples, fields.shape[3])
        out, ptrs = Engine._composite_out(fields.shape, N, residual, mse_center, epistemic=True)
        check(lib.dv_infer_fields_mc_composite(self._h, *args, int(seed), int(mc_seed), int(nsamples), *ptrs))
        return out

    # -- the same with the sub-pixel position fit and fractional placements on the GPU --
    def infer_fields_fit_composite(self, fields, starts, distances, field_ptr, seed=0, shifts=None, bound: float = 3.0,
                                   max_iter: int = 50, mc_seed=0, nsamples=0, residual=True,
                                   mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_composite() with every galaxy's sub-pixel shift fitted on the GPU (scene_fit_shifts_fields on the r
        band of the mean stamps, which stay in device memory) and the stamps placed at int((F - cs) / 2) + distances + shifts
        with scipy.ndimage.shift's cubic spline (dv_infer_fields_fit_composite).  distances (N, 2) {row, column}: integers.
        shifts (N, 2): the start (zeros by default); max_iter = 0 places at them without fitting.  nsamples > 0 adds
        infer_fields_mc_composite's "epistemic_fields" and "eps_norm".  Returns the fields and scalars of those calls plus
        {"shifts" (N, 2), "objective", "iters", "status" (N,)} as scene_fit_shifts returns them."""
        fields = _check_fields(fields)
        dist = np.ascontiguousarray(distances, dtype=np.float64).reshape(-1, 2)
        starts_c = _i32_rows(starts, "cutout starts")
        N = starts_c.shape[0]
        if dist.shape != (N, 2):
            raise ValueError(f"{N} cutout starts but distances of shape {dist.shape}")
        if not (np.isfinite(dist).all() and np.array_equal(dist, np.floor(dist)) and (np.abs(dist) <= 1e6).all()):
            raise ValueError("the device path places stamps at integer distances (within +-1e6); fractional distances need "
                             "the default path")
        if fields.shape[3] < 3:
            raise ValueError(f"the position fit uses band 2 (r); these fields have {fields.shape[3]} band(s)")
        if not (np.isfinite(bound) and 0 <= bound <= 1e6) or int(max_iter) < 0:
            raise ValueError(f"bound must lie in 0 .. 1e6 and max_iter be >= 0 (got {bound}, {max_iter})")
        sh = np.zeros((N, 2), np.float64) if shifts is None else np.array(shifts, dtype=np.float64, order="C", copy=True)
        if sh.shape != (N, 2) or not np.isfinite(sh).all() or (np.abs(sh) > 1e6).any():
            raise ValueError(f"expected finite start shifts ({N}, 2) within +-1e6, got shape {sh.shape}")
        mc = int(nsamples) != 0
        if mc:
            Engine._check_mc(nsamples, fields.shape[3])
        fields, N, args = Engine._field_args(fields, starts_c, field_ptr)
        out, ptrs = Engine._composite_out(fields.shape, N, residual, mse_center, epistemic=mc)
        if not mc:
            ptrs = ptrs[:2] + [None] + ptrs[2:] + [None]
        out.update(shifts=sh, objective=np.zeros(N, np.float64), iters=np.zeros(N, np.int32), status=np.zeros(N, np.int32))
        args = args[:5] + [_dp(dist)] + args[5:]
        check(lib.dv_infer_fields_fit_composite(self._h, *args, int(seed), float(bound), int(max_iter), _dp(sh), int(mc_seed),
                                                int(nsamples), *ptrs, _dp(out["objective"]), _ip(out["iters"]),
                                                _ip(out["status"])))
        return out

    def infer_cutouts_fit_composite(self, field, starts, distances, seed=0, **kw) -> Dict[str, np.ndarray]:
        """infer_fields_fit_composite() for one field (F, F, bands): the field-sized results under singular key names."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_fit_composite(fields, starts, distances, fp, seed=seed, **kw))

    # -- one field: M = 1 views of the calls above, the field-sized results under singular key names --
    @staticmethod
    def _one_field(field, starts):
        """(fields, starts, field_ptr) of the many-field calls for one square float64 field (F, F, bands)."""
        field = np.ascontiguousarray(field, dtype=np.float64)
        if field.ndim != 3 or field.shape[0] != field.shape[1]:
            raise ValueError(f"expected a square field (F, F, bands), got {field.shape}")
        starts = _i32_rows(starts, "cutout starts")
        return field[None], starts, [0, starts.shape[0]]

    @staticmethod
    def _singular(out):
        return {(k[:-1] if k.endswith("_fields") else k): (v[0] if k.endswith("_fields") else v) for k, v in out.items()}

    def infer_cutouts(self, field, starts, seed=0, want=("loc", "scale"), out=None) -> Dict[str, np.ndarray]:
        """infer() on the cutouts field[x:x+H, y:y+H, :] of a float64 field (F, F, bands) for every row (x, y) of `starts`,
        gathered and cast on the GPU: the stamps never visit the host.  Bit-identical to
        infer(ctx.scene_extract(field, starts, H)) with the same seed."""
        fields, starts, fp = Engine._one_field(field, starts)
        return self.infer_fields(fields, starts, fp, seed=seed, want=want, out=out)

    def infer_cutouts_keep(self, field, starts, seed=0) -> Dict[str, np.ndarray]:
        """infer_cutouts() for a caller that also needs the float64 cutouts: returns {"loc", "scale" (float32), "cutouts"
        (float64)}, all (N,) + stamp shape.  mean / stddev are bit-identical to infer(cutouts) with the same seed."""
        fields, starts, fp = Engine._one_field(field, starts)
        return self.infer_fields_keep(fields, starts, fp, seed=seed)

    def infer_cutouts_composite(self, field, starts, places, seed=0, residual=True, mse_center=True) -> Dict[str, np.ndarray]:
        """infer_fields_composite() for one field: returns {"mean_field", "stddev_field", ["residual_field"]} (F, F, bands)
        and ["mse_center"] (N,)."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_composite(fields, starts, places, fp, seed=seed, residual=residual,
                                                            mse_center=mse_center))

    def infer_cutouts_mc_keep(self, field, starts, seed=0, mc_seed=0, nsamples=100) -> Dict[str, np.ndarray]:
        """infer_cutouts_keep() plus "epistemic": infer_fields_mc_keep for one field."""
        fields, starts, fp = Engine._one_field(field, starts)
        return self.infer_fields_mc_keep(fields, starts, fp, seed=seed, mc_seed=mc_seed, nsamples=nsamples)

    def infer_cutouts_mc_composite(self, field, starts, places, seed=0, mc_seed=0, nsamples=100, residual=True,
                                   mse_center=True) -> Dict[str, np.ndarray]:
        """infer_cutouts_composite() plus "epistemic_field" and "eps_norm": infer_fields_mc_composite for one field."""
        fields, starts, fp = Engine._one_field(field, starts)
        return Engine._singular(self.infer_fields_mc_composite(fields, starts, places, fp, seed=seed, mc_seed=mc_seed,
                                                               nsamples=nsamples, residual=residual, mse_center=mse_center))

    def infer_cutouts_stream(self, field, starts, consumer, seed=0):
        """infer_cutouts() for inputs whose outputs do not belong on one host (a million cutouts: 167 GB): every finished
        chunk is handed to consumer(first, mean, stddev) - float32 views (count, H, H, bands) of the pinned transfer
        buffers, valid until the consumer returns, stamps [first, first + count) in input order.  Nothing is copied on
        the host; the GPU works on the next chunks meanwhile."""
        fields, starts, _ = Engine._one_field(field, starts)
        failure = []

        def trampoline(_user, first, count, mean_p, std_p):
            try:
                shape = (int(count),) + self.stamp_shape
                consumer(int(first), np.ctypeslib.as_array(mean_p, shape=shape), np.ctypeslib.as_array(std_p, shape=shape))
                return 0
            except BaseException as e:          # never let an exception cross the C frames
                failure.append(e)
                return 1

        cb = _lib.CHUNK_FN(trampoline)
        rc = lib.dv_infer_cutouts_stream(self._h, _dp(fields), fields.shape[1], fields.shape[3], _ip(starts), starts.shape[0],
                                         int(seed), C.cast(cb, C.c_void_p), None)
        if failure:
            raise failure[0]
        check(rc)

    def infer_mc(self, x, nsamples=100, seed=0):
        """(mean, std) over `nsamples` stochastic decodes of every stamp (encoder runs once per stamp)."""
        x = _f32c(x)
        if x.ndim != 4 or x.shape[1:] != self.stamp_shape:
            raise ValueError(f"expected images of shape (N,{self.stamp_shape}), got {x.shape}")
        mean = np.empty(x.shape, np.float32)
        std = np.empty(x.shape, np.float32)
        check(lib.dv_infer_mc(self._h, _fp(x), x.shape[0], int(nsamples), int(seed), _fp(mean), _fp(std)))
        return mean, std

    def encode(self, x) -> np.ndarray:
        x = _f32c(x)
        if x.ndim != 4 or x.shape[1:] != self.stamp_shape:
            raise ValueError(f"expected images of shape (N,{self.stamp_shape}), got {x.shape}")
        t = np.empty((x.shape[0], self.tw), np.float32)
        check(lib.dv_encode(self._h, _fp(x), x.shape[0], _fp(t)))
        return t

    def decode(self, z) -> Tuple[np.ndarray, np.ndarray]:
        z = _f32c(z)
        if z.ndim != 2 or z.shape[1] != self.latent:
            raise ValueError(f"expected latents of shape (N,{self.latent}), got {z.shape}")
        loc = np.empty((z.shape[0],) + self.stamp_shape, np.float32)
        scale = np.empty_like(loc)
        check(lib.dv_decode(self._h, _fp(z), z.shape[0], _fp(loc), _fp(scale)))
        return loc, scale

    # -- introspection ----------------------------------------------------------------------
    def activation(self, name: str, shape) -> np.ndarray:
        a = np.empty(shape, np.float32)
        check(lib.dv_model_get_activation(self._h, name.encode(), _fp(a), a.nbytes))
        return a

    def prof_enable(self, on: bool):
        check(lib.dv_prof_enable(self._h, int(on)))

    def prof_reset(self):
        check(lib.dv_prof_reset(self._h))

    def prof_families(self) -> List[Dict]:
        """[{name, launches, ms, flops, executed_flops, algorithmic_bytes}] per MFMA kernel family since the last prof_reset
        (names as rocprofv3 prints them; executed_flops: what the matrix pipe executes - Winograd kernels execute fewer
        than the direct-convolution count they are priced with)."""
        out = []
        fam = 0
        while True:
            name = C.create_string_buffer(96)
            n, ms, fl, ex, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double(), C.c_double()
            if lib.dv_prof_read_family(self._h, fam, name, 96, C.byref(n), C.byref(ms), C.byref(fl), C.byref(ex),
                                       C.byref(by)) != 0:
                break
            if n.value:
                out.append(dict(name=name.value.decode(), launches=n.value, ms=ms.value, flops=fl.value,
                                executed_flops=ex.value, algorithmic_bytes=by.value))
            fam += 1
        return out

    def prof_read(self, klass: int) -> Tuple[int, float]:
        n, ms = C.c_int64(), C.c_double()
        check(lib.dv_prof_read(self._h, klass, C.byref(n), C.byref(ms)))
        return n.value, ms.value


class FieldSet:
    """M fields resident on the GPU for an iterative deblending loop (dv_field_set_*).

    Per field the set keeps `work` (what the next pass detects on and cuts from; at first the field), `final` (the field minus
    every stamp of every pass), `mean` and `stddev` (sums over all passes).  cumulative=False: a pass's new working residual
    is the uploaded field minus the stamps of that pass only (the reference's rule); cumulative=True: every pass subtracts
    from the working residual, and `final` is `work`.  Only catalogues and per-stamp / per-field scalars cross the host link
    between passes; read() brings a stack of fields back."""

    WHICH = {"work": 0, "final": 1, "mean": 2, "stddev": 3}

    def __init__(self, engine: Engine, fields, cumulative=False):
        fields = _check_fields(fields)
        if not np.isfinite(fields).all():
            raise ValueError("the fields must be finite")
        self.engine = engine
        self.shape = fields.shape
        self.cumulative = bool(cumulative)
        self._h = C.c_void_p()
        self._rows = 0                      # stamps of the deblend_pass_measure(blend=True) calls: the set's resident rows
        self._detect_noise = None           # DV_DETECT_NOISE_* while set_detect_weights holds planes
        self._detect_bands = False          # while set_detect_bands holds a selection
        if not engine._h:
            raise RuntimeError("the Engine of this FieldSet has been closed")
        M, F, _, nb = fields.shape
        check(lib.dv_field_set_open(engine._h, _dp(fields), M, F, nb, int(self.cumulative), C.byref(self._h)))
        engine._field_sets.add(self)

    def _handle(self):
        if not self._h:
            raise _lib.DvError(-5, "the field set has been closed")
        return self._h

    def set_detect_weights(self, weights, noise=None, filter_type: str = "conv", mask=None):
        """The weight planes of every later detect() (dv_field_set_detect_weights): weights (M, F, F),
        or (M, F, F, bands) from which band 2 is taken, uploaded once and kept until close() or set_detect_weights(None),
        which goes back to the unweighted detector.  noise, filter_type and mask (M, F, F) as in Context.scene_detect.  The
        working residuals themselves must stay finite (the network reads them): fill masked pixels with finite values, the
        weights keep them out of every detection pass."""
        h = self._handle()
        M, F = self.shape[0], self.shape[1]
        if weights is None and mask is None:
            check(lib.dv_field_set_detect_weights(h, None, 0, 0))
            self._detect_noise = None
            return
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.ndim == 4:
                if weights.shape[3] <= 2:
                    raise ValueError(f"detection uses band 2; these weights have {weights.shape[3]} band(s)")
                weights = weights[:, :, :, 2]
        w, noise_id, filter_id = check_detect_weights((M, F, F), weights, mask, noise, filter_type, 1.0)
        check(lib.dv_field_set_detect_weights(h, _dp(w), noise_id, filter_id))
        self._detect_noise = noise_id

    def set_detect_bands(self, bands, band_weights=None, weights=None, mask=None, noise=None, filter_type: str = "conv"):
        """The band selection of every later detect() (dv_field_set_detect_bands): detect() then is
        Context.scene_detect_multiband on the working residuals with these bands, band_weights, planes (weights (M, F, F, k)
        and / or mask (M, F, F) or (M, F, F, k), uploaded once), noise and filter_type, and its thresh is in units of the
        combined pixel's sigma.  set_detect_bands(None) drops the selection: detect() reads band 2 again.  Refused while
        set_detect_weights holds single-band planes, and the other way round."""
        h = self._handle()
        M, F, nb = self.shape[0], self.shape[1], self.shape[3]
        if bands is None:
            check(lib.dv_field_set_detect_bands(h, None, 0, None, None, 0, 0))
            self._detect_bands = False
            return
        sel, cw = check_detect_bands(nb, bands, band_weights)
        planes, noise_id, filter_id = check_detect_band_planes((M, F, F, len(sel)), weights, mask, noise, filter_type, 1.0)
        check(lib.dv_field_set_detect_bands(h, _ip(sel), len(sel), _dp(cw), _dp(planes), noise_id, filter_id))
        self._detect_bands = True

    def set_detect_objects(self, on: bool = True, segmentation_map: bool = False):
        """Every later detect() also returns the columns of Context.scene_detect_objects (dv_field_set_detect_objects,
        DESIGN.md section 7zb), with segmentation_map also segmap (M, F, F), 0 in fields that were not active.
        set_detect_objects(False) goes back to the catalogue alone.  While on, detect() refuses thresh < 0."""
        check(lib.dv_field_set_detect_objects(self._handle(), int(bool(on)), int(bool(on) and bool(segmentation_map))))
        self._detect_objects = (bool(on), bool(on) and bool(segmentation_map))

    def set_detect_clean(self, on: bool = True, clean_param: float = 1.0):
        """Every later detect() runs the cleaning pass of Context.scene_detect_clean with clean_param
        (dv_field_set_detect_clean) and returns the cleaned catalogue with nmerged, mthresh and n_raw
        (M,), 0 for a field that was not active; the columns of set_detect_objects are then the cleaned ones.
        set_detect_clean(False) goes back to the detection as it was.  While on, detect() refuses thresh <= 0 and
        minarea > 64."""
        if on:
            check_detect_clean(clean_param, None, None)
        check(lib.dv_field_set_detect_clean(self._handle(), int(bool(on)), float(clean_param) if on else 1.0))
        self._detect_clean = bool(on)

    def detect(self, active=None, thresh: float = 1.5, minarea: int = 4, nthresh: int = 64, cont: float = 1e-5,
               filter_kernel=None, back_size: int = 64, back_filter: int = 3, workspace_bytes: int = 0) -> Dict[str, np.ndarray]:
        """Context.scene_detect on band 2 of the working residuals, which do not leave the GPU (dv_field_set_detect).
        active: (M,) booleans, None for all fields; an inactive field gets an empty catalogue range.  Returns the
        catalogue, offsets (M + 1,) and globalrms (M,) of scene_detect, without maps, in the set's field numbering; after
        set_detect_objects also the columns of Context.scene_detect_objects."""
        h = self._handle()
        M, F = self.shape[0], self.shape[1]
        objects_on, segmap_on = getattr(self, "_detect_objects", (False, False))
        if objects_on and not float(thresh) >= 0:
            raise ValueError(f"with the object columns on thresh must be >= 0, got {thresh}")
        clean_on = getattr(self, "_detect_clean", False)
        if clean_on:
            check_detect_clean(1.0, thresh, minarea)
        check_detect_args(np.zeros((0, F, F)), thresh, minarea, nthresh, cont, filter_kernel, back_size, back_filter,
                          workspace_bytes)
        if getattr(self, "_detect_noise", None) == _lib.DETECT_NOISE["absolute"] and not float(thresh) > 0:
            raise ValueError(f"with noise='absolute' thresh is in units of the pixel's sigma and must be > 0, got {thresh}")
        if getattr(self, "_detect_bands", False) and not float(thresh) > 0:
            raise ValueError(f"with a band selection thresh is in units of the combined pixel's sigma and must be > 0, got {thresh}")
        act = None
        if active is not None:
            act = np.ascontiguousarray(np.asarray(active, dtype=bool).astype(np.uint8))
            if act.shape != (M,):
                raise ValueError(f"expected one active flag per field ({M}), got shape {act.shape}")
        params, kern = _detect_params(thresh, cont, minarea, nthresh, back_size, back_filter, filter_kernel, workspace_bytes)

        def call(cap, n, offsets, grms, columns):
            check(lib.dv_field_set_detect(h, None if act is None else act.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          C.byref(params), cap, n, offsets, grms, *columns))

        out, rows = _run_detect(M, F * F, call)
        if objects_on:
            obj, ostruct = _object_buffers(rows, (M, F, F) if segmap_on else None)
            check(lib.dv_field_set_detect_objects_read(h, rows, C.byref(ostruct)))
            out.update(obj)
            out.update(detect_object_shapes(out["x2"], out["y2"], out["xy"]))
        if clean_on:
            cl = dict(nmerged=np.zeros(rows, np.int32), mthresh=np.zeros(rows, np.float64), n_raw=np.zeros(M, np.int64))
            check(lib.dv_field_set_detect_clean_read(h, rows, _ip(cl["nmerged"]), _dp(cl["mthresh"]),
                                                     cl["n_raw"].ctypes.data_as(C.POINTER(C.c_int64))))
            out.update(cl)
        return out

    def deblend_pass(self, starts, places, field_ptr, seed=0) -> Dict[str, np.ndarray]:
        """One deblending pass over the stamps of all fields (dv_field_set_pass): starts / places (N, 2) and field_ptr
        (M + 1,) as in Engine.infer_fields_composite, the stamps being cut from the working residuals as they are before
        the pass.  Returns {"mse_center" (N,), "field_mse" (M,)}: field_mse[m] = mean((work - work_new)^2) of a field that
        has stamps, NaN for a field without (which the pass does not touch)."""
        h = self._handle()
        starts = _i32_rows(starts, "cutout starts")
        places = _i32_rows(places, "stamp placements")
        if places.shape != starts.shape:
            raise ValueError(f"{starts.shape[0]} cutout starts but {places.shape[0]} placements")
        N = starts.shape[0]
        fp = check_field_ptr(field_ptr, self.shape[0], N)
        mse_center = np.empty(N, np.float64)
        field_mse = np.full(self.shape[0], np.nan)
        check(lib.dv_field_set_pass(h, _ip(starts), _ip(places), fp.ctypes.data_as(C.POINTER(C.c_int64)), N, int(seed),
                                    _dp(mse_center), _dp(field_mse)))
        return {"mse_center": mse_center, "field_mse": field_mse}

    def deblend_pass_measure(self, starts, places, field_ptr, seed=0, band: int = 2, sigma0: float = 3.0, tol: float = 1e-10,
                             max_iter: int = 200, blend=True) -> Dict[str, np.ndarray]:
        """deblend_pass() with every stamp measured where it lies in device memory (dv_field_set_pass_measure, DESIGN.md
        section 7m).  Returns deblend_pass's dictionary, bit for bit, plus {"flux", "flux_err" (N, bands), "shape" (N, 5),
        "iters", "status" (N,)} - the bits of Context.scene_measure on the stamps Engine.infer_fields returns for the working
        residuals and the same seed - and, with blend=True, {"child" (N, 2) = {W, A}, "npix" (N,)}: the stamp sums of
        Context.scene_blend.  With blend=True the set also keeps every stamp's shape, status, placement and field on the
        device, in call order over all passes: the rows blend_sums() works on."""
        h = self._handle()
        starts = _i32_rows(starts, "cutout starts")
        places = _i32_rows(places, "stamp placements")
        if places.shape != starts.shape:
            raise ValueError(f"{starts.shape[0]} cutout starts but {places.shape[0]} placements")
        N = starts.shape[0]
        fp = check_field_ptr(field_ptr, self.shape[0], N)
        nb = self.shape[3]
        par = measure_params(band, sigma0, tol, max_iter, nb)
        cs = self.engine.stamp_shape[0]
        if cs > MEASURE_MAX_STAMP:
            raise ValueError(f"stamps of {cs} pixels: the measurement takes at most {MEASURE_MAX_STAMP}")
        out = {"mse_center": np.empty(N, np.float64), "field_mse": np.full(self.shape[0], np.nan),
               "flux": np.zeros((N, nb), np.float64), "flux_err": np.zeros((N, nb), np.float64),
               "shape": np.zeros((N, 5), np.float64), "iters": np.zeros(N, np.int32), "status": np.zeros(N, np.int32)}
        if blend:
            out.update(child=np.zeros((N, 2), np.float64), npix=np.zeros(N, np.int32))
        check(lib.dv_field_set_pass_measure(h, _ip(starts), _ip(places), fp.ctypes.data_as(C.POINTER(C.c_int64)), N, int(seed),
                                            C.byref(par), _dp(out["mse_center"]), _dp(out["field_mse"]), _dp(out["flux"]),
                                            _dp(out["flux_err"]), _dp(out["shape"]), _ip(out["iters"]), _ip(out["status"]),
                                            _dp(out.get("child")), _ip(out["npix"]) if blend else None))
        if blend:
            self._rows += N
        return out

    def blend_sums(self, band: int = 2) -> np.ndarray:
        """(Ntot, 4) float64 {Bm, Bd, R1, R2} for the Ntot stamps of all deblend_pass_measure(blend=True) calls so far, in call
        order, against the set's stacks as they are now (dv_field_set_blend): under the Gaussian weight g of a stamp's
        adaptive moments and over its pixels inside the field, Bm = sum g mean, Bd = sum g base (the field as uploaded; NaN
        on every row of a cumulative set, which keeps no base), R1 = sum g final, R2 = sum g final^2.  An ineligible row
        (Context.scene_blend's rule) gets four NaN."""
        h = self._handle()
        if int(band) != band or not 0 <= int(band) < self.shape[3]:
            raise ValueError(f"band {band} asked for, the fields have bands 0 .. {self.shape[3] - 1}")
        sums = np.zeros((self._rows, 4), np.float64)
        check(lib.dv_field_set_blend(h, int(band), self._rows, _dp(sums)))
        return sums

    def keep_stamps(self, on: bool = True):
        """From now on every deblend_pass_measure(blend=True) call also keeps its float32 mean stamps on the device, each at its
        resident row number (dv_field_set_keep_stamps): what fit_flux() works on.  Allowed only before
        the first such pass (DvError, DV_E_STATE, afterwards)."""
        check(lib.dv_field_set_keep_stamps(self._handle(), int(bool(on))))

    def _fit_flux_args(self, data_fields, weight_fields):
        """What fit_flux() and fit_flux_groups() share: the checked float64 data and weight fields (None where not given) and
        the per-row result dictionary with its pointers in the C-ABI's order, fit_chi2 / fit_npix NULL without weights."""
        data = None
        if data_fields is not None:
            data = np.ascontiguousarray(data_fields, dtype=np.float64)
            if data.shape != tuple(self.shape):
                raise ValueError(f"expected data fields of the shape of the set's fields {tuple(self.shape)}, got {data.shape}")
        elif self.cumulative:
            raise ValueError("a cumulative set keeps no copy of the fields as uploaded: give data_fields")
        weights = None if weight_fields is None else check_fit_weights(weight_fields, self.shape)
        out, ptrs = _fit_flux_out(self._rows, self.shape[3], weights is not None)
        if weights is None:
            ptrs += [None, None]
        return data, weights, out, ptrs

    def fit_flux(self, data_fields=None, weight_fields=None, sky_order=None, nonneg=False, min_pivot: float = 1e-8,
                 max_iter: int = 100, scratch_bytes: int = 256 << 20) -> Dict[str, np.ndarray]:
        """The joint flux fit of the stamps of ALL deblend_pass_measure(blend=True) calls since keep_stamps(), one linear system
        per field and band, on stamps that never left the GPU (dv_field_set_fit_flux).  Inside a field the
        galaxies stand pass after pass, each pass in its own order: of two models that cannot be told apart the copy from the
        later pass is dropped (fit_status 5, fit_scale 1).  data_fields (M, F, F, bands): what the models are fitted to; None:
        the fields as uploaded, which only a set with cumulative=False keeps.  weight_fields, sky_order (None: no sky), nonneg,
        min_pivot, max_iter and scratch_bytes are those of Context.scene_fit_flux, scene_fit_flux_sky and
        scene_fit_flux_nonneg, and the dictionary has the keys of the one of them the arguments choose - the per-galaxy arrays
        (Ntot, bands) in call order, like blend_sums(); the sky arrays and nonneg_iters / nonneg_status per field - with the
        bits of that call on the same stamps regrouped field by field.  The set is only read: the call may be repeated.  A set
        without resident rows fits nothing, no sky either: the per-field arrays come back as zeros."""
        h = self._handle()
        M, F, _, nb = self.shape
        data, weights, out, ptrs = self._fit_flux_args(data_fields, weight_fields)
        sky, order, sky_ptrs = _fit_sky_args(sky_order, M, nb)
        par = fit_flux_params(min_pivot, scratch_bytes)
        nonneg = bool(nonneg)
        max_iter = nonneg_max_iter(max_iter) if nonneg else 1
        n = self._rows
        out.update(sky)
        nn_ptrs = [None] * 5
        if nonneg:
            nn, nn_ptrs = _fit_nonneg_out(n, M, nb)
            out.update(nn)
        check(lib.dv_field_set_fit_flux(h, n, None if data is None else _dp(data), None if weights is None else _dp(weights),
                                        order, int(nonneg), C.byref(par), max_iter, *ptrs, *sky_ptrs, *nn_ptrs))
        return out

    def fit_flux_groups(self, data_fields=None, weight_fields=None, min_pivot: float = 1e-8,
                        scratch_bytes: int = 256 << 20) -> Dict[str, np.ndarray]:
        """fit_flux() by blend groups (dv_field_set_fit_flux_groups): the rows of all passes in the joint
        order of fit_flux() - field by field, inside a field pass after pass -, the connected components of their overlap graph
        found on the GPU and each solved on its own, in place on the stamp store.  A field may hold any number of rows over its
        passes; a group of more than 1024, or whose bands x n_g x n_g doubles exceed scratch_bytes, is refused by name and the
        set stays usable.  data_fields and weight_fields as in fit_flux(); no sky, no constraint.  The dictionary is
        Context.scene_fit_flux_groups's, the per-galaxy arrays in call order: "fit_group" (Ntot,) int32 is the smallest row of
        the galaxy's group counted from the field's first row in the joint order - an index into the field's rows concatenated
        pass after pass -, "fit_group_size" the members of that group.  The bits are those of scene_fit_flux_groups on the same
        stamps regrouped field by field, and of fit_flux() wherever that call takes the field."""
        h = self._handle()
        data, weights, out, ptrs = self._fit_flux_args(data_fields, weight_fields)
        par = fit_flux_params(min_pivot, scratch_bytes)
        n = self._rows
        out["fit_group"], out["fit_group_size"] = np.zeros(n, np.int32), np.zeros(n, np.int32)
        check(lib.dv_field_set_fit_flux_groups(h, n, None if data is None else _dp(data), None if weights is None else _dp(weights),
                                               C.byref(par), *ptrs, _ip(out["fit_group"]), _ip(out["fit_group_size"])))
        return out

    def read(self, which: str) -> np.ndarray:
        """One of the set's stacks as (M, F, F, bands) float64: "work", "final", "mean" or "stddev"."""
        h = self._handle()
        if which not in self.WHICH:
            raise ValueError(f"which must be one of {sorted(self.WHICH)}, got {which!r}")
        out = np.empty(self.shape, np.float64)
        check(lib.dv_field_set_read(h, self.WHICH[which], _dp(out)))
        return out

    def close(self):
        """Frees the set's device memory.  Idempotent; any other call on a closed set raises DvError (DV_E_STATE)."""
        if self._h:
            lib.dv_field_set_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
