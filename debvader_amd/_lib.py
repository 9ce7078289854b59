"""ctypes binding of libdebvader_hip.so (include/debvader_hip.h).

The library is the product: there is no CPU or PyTorch fallback.  If it is missing or fails to load,
importing this module raises with the build command to run.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DEBVADER_AMD_LIB selects another build of the same library (the host-side AddressSanitizer build, `make asan`)
LIB_PATH = os.environ.get("DEBVADER_AMD_LIB") or os.path.join(_HERE, "lib", "libdebvader_hip.so")

DV_MAX_LEVELS = 8
DV_UNIQUE_ID_BYTES = 128
DV_N_SCALARS = 4
SCALAR_NAMES = ("loss", "nll_mean", "kl_reg", "mse")


class DvConfig(C.Structure):
    _fields_ = [
        ("height", C.c_int32), ("width", C.c_int32), ("bands", C.c_int32),
        ("latent_dim", C.c_int32), ("n_levels", C.c_int32),
        ("filters", C.c_int32 * DV_MAX_LEVELS), ("kernels", C.c_int32 * DV_MAX_LEVELS),
        ("max_batch", C.c_int32),
        ("kl_weight", C.c_float), ("kl_multiplicity", C.c_int32),
        ("bn_eps", C.c_float), ("bn_momentum", C.c_float), ("bn_moving_var_unbiased", C.c_int32),
        ("sigma_floor", C.c_float), ("diag_shift", C.c_float),
        ("dtype", C.c_int32),
        ("infer_graph", C.c_int32),
    ]


DV_DTYPE_F32, DV_DTYPE_BF16 = 0, 1


class DvDetectParams(C.Structure):
    """dv_detect_params (include/debvader_hip.h)"""
    _fields_ = [
        ("thresh", C.c_double), ("cont", C.c_double),
        ("minarea", C.c_int32), ("nthresh", C.c_int32), ("back_size", C.c_int32), ("back_filter", C.c_int32),
        ("kernel", C.POINTER(C.c_double)), ("kh", C.c_int32), ("kw", C.c_int32),
        ("workspace_bytes", C.c_int64),
    ]


class DvDetectWeights(C.Structure):
    """dv_detect_weights (include/debvader_hip.h)"""
    _fields_ = [("weights", C.POINTER(C.c_double)), ("noise", C.c_int32), ("filter", C.c_int32)]


class DvDetectBands(C.Structure):
    """dv_detect_bands (include/debvader_hip.h)"""
    _fields_ = [("bands", C.POINTER(C.c_int32)), ("k", C.c_int32), ("band_weights", C.POINTER(C.c_double)),
                ("planes", C.POINTER(C.c_double)), ("noise", C.c_int32), ("filter", C.c_int32)]


# the columns of dv_detect_objects in the struct's order
DETECT_OBJECT_INT = ("xmin", "xmax", "ymin", "ymax", "xpeak", "ypeak", "xvpeak", "yvpeak", "flag")
DETECT_OBJECT_DOUBLE = ("vpeak", "dflux", "x_iso", "y_iso", "x2", "y2", "xy")
DETECT_FLAG_BLENDED, DETECT_FLAG_BORDER, DETECT_FLAG_SINGULAR, DETECT_FLAG_MASKED = 1, 2, 4, 8    # DV_DETECT_FLAG_*


class DvDetectObjects(C.Structure):
    """dv_detect_objects (include/debvader_hip.h)"""
    _fields_ = ([(k, C.POINTER(C.c_int32)) for k in DETECT_OBJECT_INT]
                + [(k, C.POINTER(C.c_double)) for k in DETECT_OBJECT_DOUBLE] + [("segmap", C.POINTER(C.c_int32))])


DETECT_FLAG_MERGED = 16                           # DV_DETECT_FLAG_MERGED
DETECT_CLEAN_MINAREA_MAX = 64                     # the cleaning pass takes minarea up to this


class DvDetectClean(C.Structure):
    """dv_detect_clean (include/debvader_hip.h)"""
    _fields_ = [("clean_param", C.c_double), ("nmerged", C.POINTER(C.c_int32)), ("mthresh", C.POINTER(C.c_double)),
                ("n_raw", C.POINTER(C.c_int64))]


DETECT_NOISE = {"absolute": 0, "relative": 1}     # DV_DETECT_NOISE_*
DETECT_FILTER = {"conv": 0, "matched": 1}         # DV_DETECT_FILTER_*


class DvMeasureParams(C.Structure):
    """dv_measure_params (include/debvader_hip.h)"""
    _fields_ = [("band", C.c_int32), ("sigma0", C.c_double), ("tol", C.c_double), ("max_iter", C.c_int32)]


class DvApertureParams(C.Structure):
    """dv_aperture_params (include/debvader_hip.h)"""
    _fields_ = [("n_radii", C.c_int32), ("n_fractions", C.c_int32), ("subsample", C.c_int32), ("bisect_iters", C.c_int32),
                ("radii", C.c_double * 8), ("fractions", C.c_double * 4), ("kron_factor", C.c_double), ("kron_min", C.c_double),
                ("kron_limit", C.c_double)]


class DvFitFluxParams(C.Structure):
    """dv_fit_flux_params (include/debvader_hip.h)"""
    _fields_ = [("min_pivot", C.c_double), ("scratch_bytes", C.c_int64)]


class DvError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"libdebvader_hip status {status}: {msg}")
        self.status = status


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP engine first "
            "(python -c 'import __graft_entry__ as g; g.build()'  or  make -C debvader_amd/csrc). "
            "debvader_amd has no CPU fallback.")
    try:
        return C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover
        raise ImportError(f"could not load {LIB_PATH}: {e}") from e


lib = _load()

_p = C.c_void_p
_f = C.POINTER(C.c_float)
_d = C.POINTER(C.c_double)
_i32 = C.POINTER(C.c_int32)
_i64 = C.POINTER(C.c_int64)

# name -> (restype, argtypes); every symbol declared in include/debvader_hip.h
# dv_chunk_fn of dv_infer_cutouts_stream: int (*)(void* user, int64 first, int32 count, const float* mean, const float* stddev)
CHUNK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float))

# the arguments every dv_infer_fields_measure* call shares: the model to seed, then params, the three result fields,
# mse_center and the five catalogue rows; the Monte-Carlo call has mc_seed and nsamples between the two, and the outputs of
# an extra follow
_FIELDS_IN = [_p, _d, C.c_int32, C.c_int32, C.c_int32, _i32, _i32, _i64, C.c_int64, C.c_uint64]
_MEASURE_OUT = [C.POINTER(DvMeasureParams), _d, _d, _d, _d, _d, _d, _d, _i32, _i32]
_APER_OUT = [C.POINTER(DvApertureParams), _d, _d, _d, _d, _d, _d, _d, _i32, _i32]


def _measure_sig(*extra, between=()):
    return C.c_int, _FIELDS_IN + list(between) + _MEASURE_OUT + list(extra)


SIGNATURES = {
    "dv_version": (C.c_int, []),
    "dv_build_kind": (C.c_int, []),
    "dv_crc32c": (C.c_uint32, [C.c_uint32, C.c_void_p, C.c_size_t]),
    "dv_last_error": (C.c_int, [C.c_char_p, C.c_size_t]),
    "dv_config_default": (C.c_int, [C.POINTER(DvConfig)]),
    "dv_arch_counts": (C.c_int, [C.POINTER(DvConfig), _i32, _i64, _i64, _i64]),
    "dv_arch_describe": (C.c_int, [C.POINTER(DvConfig), C.c_int32, C.c_char_p, C.c_size_t, _i64, _i32, _i32]),
    "dv_arch_macs": (C.c_int, [C.POINTER(DvConfig), _i64, _i64]),
    "dv_arch_buckets": (C.c_int, [C.POINTER(DvConfig), C.POINTER(C.c_int64)]),
    "dv_arch_offset": (C.c_int, [C.POINTER(DvConfig), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "dv_device_count": (C.c_int, [_i32]),
    "dv_device_bus_id": (C.c_int, [C.c_int32, C.c_char_p, C.c_size_t]),
    "dv_comm_unique_id": (C.c_int, [_p]),
    "dv_ctx_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _p, C.POINTER(_p)]),
    "dv_ctx_destroy": (C.c_int, [_p]),
    "dv_ctx_sync": (C.c_int, [_p]),
    "dv_ctx_allreduce_host": (C.c_int, [_p, _f, C.c_int32]),
    "dv_ctx_comm_info": (C.c_int, [_p, _i32, _i32, _i32, C.c_char_p, C.c_size_t, _i32]),
    "dv_comm_prof_enable": (C.c_int, [_p, C.c_int32]),
    "dv_comm_prof_read": (C.c_int, [_p, _i64, C.POINTER(C.c_double), _i64, C.POINTER(C.c_double)]),
    "dv_model_create": (C.c_int, [_p, C.POINTER(DvConfig), C.POINTER(_p)]),
    "dv_model_destroy": (C.c_int, [_p]),
    "dv_model_init": (C.c_int, [_p, C.c_uint64]),
    "dv_model_get_param": (C.c_int, [_p, C.c_int32, _f, C.c_size_t]),
    "dv_model_set_param": (C.c_int, [_p, C.c_int32, _f, C.c_size_t]),
    "dv_model_get_grad": (C.c_int, [_p, C.c_int32, _f, C.c_size_t]),
    "dv_model_get_slot": (C.c_int, [_p, C.c_int32, C.c_int32, _f, C.c_size_t]),
    "dv_model_set_slot": (C.c_int, [_p, C.c_int32, C.c_int32, _f, C.c_size_t]),
    "dv_model_set_trainable": (C.c_int, [_p, C.c_int32, C.c_int32]),
    "dv_optimizer_reset": (C.c_int, [_p, C.c_float, C.c_float, C.c_float, C.c_float]),
    "dv_optimizer_get_iter": (C.c_int, [_p, _i64]),
    "dv_optimizer_set_iter": (C.c_int, [_p, C.c_int64]),
    "dv_data_upload": (C.c_int, [_p, C.c_int32, _f, _f, C.c_int64]),
    "dv_data_free": (C.c_int, [_p, C.c_int32]),
    "dv_data_stream_open": (C.c_int, [_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                      C.c_int64]),
    "dv_data_info": (C.c_int, [_p, C.c_int32, _i32, _i64, _i64]),
    "dv_ctx_mem_info": (C.c_int, [_p, _i64, _i64]),
    "dv_train_step": (C.c_int, [_p, C.c_int32, _i32, C.c_int64, C.c_int32, C.c_int32, _f, C.c_uint64, _f]),
    "dv_eval_step": (C.c_int, [_p, C.c_int32, _i32, C.c_int64, C.c_int32, C.c_int32, _f, C.c_uint64, _f]),
    "dv_grad_step": (C.c_int, [_p, C.c_int32, _i32, C.c_int64, C.c_int32, C.c_int32, _f, C.c_uint64, _f]),
    "dv_train_step_async": (C.c_int, [_p, C.c_int32, C.POINTER(C.c_int32), C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int32]),
    "dv_step_result": (C.c_int, [_p, C.c_int32, _f]),
    "dv_train_steps": (C.c_int, [_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _f]),
    "dv_model_set_normalise": (C.c_int, [_p, C.c_int32]),
    "dv_model_set_mse_sample": (C.c_int, [_p, C.c_int32]),
    "dv_model_set_keep_outputs": (C.c_int, [_p, C.c_int32]),
    "dv_infer": (C.c_int, [_p, _f, C.c_int64, _f, C.c_uint64, _f, _f, _f, _f, _f]),
    "dv_infer_f64": (C.c_int, [_p, _d, C.c_int64, _f, C.c_uint64, _f, _f, _f, _f, _f]),
    "dv_infer_cutouts": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int64, C.c_uint64, _f, _f, _f, _f, _f]),
    "dv_infer_cutouts_keep": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int64, C.c_uint64, _f, _f, _d]),
    "dv_infer_cutouts_stream": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int64, C.c_uint64,
                                          C.c_void_p, C.c_void_p]),
    "dv_infer_cutouts_composite": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64,
                                             C.c_uint64, _d, _d, _d, _d]),
    "dv_infer_fields": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, _i32, _i64, C.c_int64, C.c_uint64, _f, _f, _f, _f, _f]),
    "dv_infer_fields_keep": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, _i32, _i64, C.c_int64, C.c_uint64, _f, _f, _f, _f,
                                       _f, _d]),
    "dv_infer_fields_composite": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, _i32, _i32, _i64, C.c_int64, C.c_uint64,
                                            _d, _d, _d, _d]),
    "dv_infer_fields_mc_keep": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, _i32, _i64, C.c_int64, C.c_uint64, C.c_uint64,
                                          C.c_int32, _f, _f, _d, _f]),
    "dv_infer_fields_mc_composite": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, _i32, _i32, _i64, C.c_int64, C.c_uint64,
                                               C.c_uint64, C.c_int32, _d, _d, _d, _d, _d, _d]),
    "dv_infer_fields_fit_composite": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, _i32, _d, _i64, C.c_int64, C.c_uint64,
                                                C.c_double, C.c_int32, _d, C.c_uint64, C.c_int32, _d, _d, _d, _d, _d, _d, _d,
                                                _i32, _i32]),
    "dv_scene_extract": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, _d]),
    "dv_scene_composite": (C.c_int, [_p, _d, C.c_int32, C.c_int32, _d, _d, C.c_int32, C.c_int32, C.c_double]),
    "dv_scene_fit_shifts": (C.c_int, [_p, _d, C.c_int32, _d, C.c_int32, C.c_int32, _d, C.c_double, C.c_int32, _d, _d,
                                      _i32, _i32]),
    "dv_scene_fit_shifts_fields": (C.c_int, [_p, _d, C.c_int32, C.c_int32, _d, _i64, C.c_int64, C.c_int32, _d, C.c_double,
                                             C.c_int32, _d, _d, _i32, _i32]),
    "dv_scene_detect": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DvDetectParams), C.c_int64, _i64,
                                  _i64, _d, _i32, _i32, _i32, _d, _d, _d, _d, _d, _d, _d, _i32]),
    "dv_scene_detect_weighted": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DvDetectParams), C.c_int64, _i64,
                                           _i64, _d, _i32, _i32, _i32, _d, _d, _d, _d, _d, _d, _d, _i32,
                                           C.POINTER(DvDetectWeights), _i32]),
    "dv_scene_detect_multiband": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DvDetectParams),
                                            C.c_int64, _i64, _i64, _d, _i32, _i32, _i32, _d, _d, _d, _d, _d, _d, _d, _d, _d, _i32,
                                            C.POINTER(DvDetectBands), _d, _i32]),
    "dv_scene_detect_objects": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DvDetectParams),
                                          C.c_int64, _i64, _i64, _d, _i32, _i32, _i32, _d, _d, _d, _d,
                                          C.POINTER(DvDetectWeights), C.POINTER(DvDetectBands), C.POINTER(DvDetectObjects)]),
    "dv_scene_detect_clean": (C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DvDetectParams),
                                        C.c_int64, _i64, _i64, _d, _i32, _i32, _i32, _d, _d, _d, _d,
                                        C.POINTER(DvDetectWeights), C.POINTER(DvDetectBands), C.POINTER(DvDetectObjects),
                                        C.POINTER(DvDetectClean)]),
    "dv_measure_params_default": (C.c_int, [C.POINTER(DvMeasureParams)]),
    "dv_scene_measure": (C.c_int, [_p, _f, _f, C.c_int64, C.c_int32, C.c_int32, C.POINTER(DvMeasureParams), _d, _d, _d, _i32,
                                   _i32]),
    "dv_infer_fields_measure": _measure_sig(),
    "dv_scene_measure_mc": (C.c_int, [_p, _f, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(DvMeasureParams), _d, _d, _d,
                                      _d, _i32, _d, _d, _i32]),
    "dv_infer_fields_measure_mc": _measure_sig(_d, _d, _d, _d, _i32, _d, _d, _i32, between=(C.c_uint64, C.c_int32)),
    "dv_scene_blend": (C.c_int, [_p, _f, _d, _i32, _i32, _i64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _d, _d, C.c_int32,
                                 C.c_int32, _d, _i32]),
    "dv_infer_fields_measure_blend": _measure_sig(_d, _i32),
    "dv_scene_regauss": (C.c_int, [_p, _f, _d, _i32, _i32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _d, C.c_int32, C.c_int32,
                                   C.c_double, C.c_double, C.c_int32, _d, _i32, _i32, _d, _d, _i32, _i32]),
    "dv_infer_fields_measure_psf": _measure_sig(_d, C.c_int32, C.c_int32, _i32, C.c_double, _d, _i32, _i32, _d, _d, _i32, _i32),
    "dv_aperture_params_default": (C.c_int, [C.POINTER(DvApertureParams)]),
    "dv_scene_aperture": (C.c_int, [_p, _f, _f, _d, _i32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DvApertureParams),
                                    _d, _d, _d, _d, _d, _d, _d, _i32, _i32]),
    "dv_infer_fields_measure_aper": _measure_sig(*_APER_OUT),
    "dv_scene_aperture_fields": (C.c_int, [_p, _d, _i32, _i32, _i64, _d, _i32, C.c_int64, C.c_int32, C.c_int32, _d, _d, C.c_int32,
                                           C.c_int32, C.POINTER(DvApertureParams), _d, _d, _d, _d, _d, _d]),
    "dv_infer_fields_measure_aper_data": _measure_sig(*_APER_OUT, _d, _d, _d, _d, _d, _d),
    "dv_fit_flux_params_default": (C.c_int, [C.POINTER(DvFitFluxParams)]),
    "dv_scene_fit_flux": (C.c_int, [_p, _f, _i32, _i64, C.c_int64, C.c_int32, C.c_int32, _d, C.c_int32, C.c_int32,
                                    C.POINTER(DvFitFluxParams), _d, _d, _d, _d, _i32]),
    "dv_scene_fit_flux_gram": (C.c_int, [_p, _f, _i32, C.c_int64, C.c_int32, C.c_int32, _d, C.c_int32, _d, _d]),
    "dv_infer_fields_measure_fit": _measure_sig(C.POINTER(DvFitFluxParams), _d, _d, _d, _d, _i32),
    "dv_scene_fit_flux_weighted": (C.c_int, [_p, _f, _i32, _i64, C.c_int64, C.c_int32, C.c_int32, _d, _d, C.c_int32, C.c_int32,
                                             C.POINTER(DvFitFluxParams), _d, _d, _d, _d, _i32, _d, _i32]),
    "dv_infer_fields_measure_fit_weighted": _measure_sig(C.POINTER(DvFitFluxParams), _d, _d, _d, _d, _d, _i32, _d, _i32),
    "dv_scene_fit_flux_groups": (C.c_int, [_p, _f, _i32, _i64, C.c_int64, C.c_int32, C.c_int32, _d, C.c_int32, C.c_int32,
                                           C.POINTER(DvFitFluxParams), _d, _d, _d, _d, _d, _i32, _d, _i32, _i32, _i32]),
    "dv_infer_fields_measure_fit_groups": _measure_sig(C.POINTER(DvFitFluxParams), _d, _d, _d, _d, _d, _i32, _d, _i32, _i32, _i32),
    "dv_scene_fit_groups": (C.c_int, [_p, _i32, _i64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _i32, _i32, C.c_int64, _i64,
                                      _i32, C.c_int64, _i64, _i32, _i32]),
    "dv_scene_fit_flux_sky": (C.c_int, [_p, _f, _i32, _i64, C.c_int64, C.c_int32, C.c_int32, _d, _d, C.c_int32, C.c_int32,
                                        C.POINTER(DvFitFluxParams), C.c_int32, _d, _d, _d, _d, _i32, _d, _i32, _d, _d, _i32, _i64]),
    "dv_scene_fit_flux_sky_gram": (C.c_int, [_p, _f, _i32, C.c_int64, C.c_int32, C.c_int32, _d, _d, C.c_int32, C.c_int32, _d, _d]),
    "dv_infer_fields_measure_fit_sky": _measure_sig(C.POINTER(DvFitFluxParams), _d, C.c_int32, _d, _d, _d, _d, _i32, _d, _i32,
                                                    _d, _d, _i32, _i64),
    "dv_scene_fit_flux_nonneg": (C.c_int, [_p, _f, _i32, _i64, C.c_int64, C.c_int32, C.c_int32, _d, _d, C.c_int32, C.c_int32,
                                           C.POINTER(DvFitFluxParams), C.c_int32, C.c_int32, _d, _d, _d, _d, _i32, _d, _i32,
                                           _d, _d, _i32, _i64, _d, _i32, _d, _i32, _i32]),
    "dv_infer_fields_measure_fit_nonneg": _measure_sig(C.POINTER(DvFitFluxParams), _d, C.c_int32, C.c_int32, _d, _d, _d, _d, _i32,
                                                       _d, _i32, _d, _d, _i32, _i64, _d, _i32, _d, _i32, _i32),
    "dv_scene_moments_fields": (C.c_int, [_p, _f, _i32, _i64, C.c_int64, C.c_int32, C.c_int32, _d, _d, _d, C.c_int32, C.c_int32,
                                          C.POINTER(DvMeasureParams), _d, _i32, _d, _i32, _i32]),
    "dv_infer_fields_measure_moments_data": _measure_sig(_d, _d, _i32, _d, _i32, _i32),
    "dv_field_set_open":(C.c_int, [_p, _d, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_p)]),
    "dv_field_set_detect": (C.c_int, [_p, C.POINTER(C.c_uint8), C.POINTER(DvDetectParams), C.c_int64, _i64, _i64, _d, _i32,
                                      _i32, _i32, _d, _d, _d, _d]),
    "dv_field_set_detect_weights": (C.c_int, [_p, _d, C.c_int32, C.c_int32]),
    "dv_field_set_detect_bands": (C.c_int, [_p, _i32, C.c_int32, _d, _d, C.c_int32, C.c_int32]),
    "dv_field_set_detect_objects": (C.c_int, [_p, C.c_int32, C.c_int32]),
    "dv_field_set_detect_objects_read": (C.c_int, [_p, C.c_int64, C.POINTER(DvDetectObjects)]),
    "dv_field_set_detect_clean": (C.c_int, [_p, C.c_int32, C.c_double]),
    "dv_field_set_detect_clean_read": (C.c_int, [_p, C.c_int64, _i32, _d, _i64]),
    "dv_field_set_pass": (C.c_int, [_p, _i32, _i32, _i64, C.c_int64, C.c_uint64, _d, _d]),
    "dv_field_set_read": (C.c_int, [_p, C.c_int32, _d]),
    "dv_field_set_close": (C.c_int, [_p]),
    "dv_field_set_pass_measure": (C.c_int, [_p, _i32, _i32, _i64, C.c_int64, C.c_uint64, C.POINTER(DvMeasureParams), _d, _d, _d,
                                            _d, _d, _i32, _i32, _d, _i32]),
    "dv_field_set_blend": (C.c_int, [_p, C.c_int32, C.c_int64, _d]),
    "dv_field_set_keep_stamps": (C.c_int, [_p, C.c_int32]),
    "dv_field_set_fit_flux": (C.c_int, [_p, C.c_int64, _d, _d, C.c_int32, C.c_int32, C.POINTER(DvFitFluxParams), C.c_int32,
                                        _d, _d, _d, _d, _i32, _d, _i32, _d, _d, _i32, _i64, _d, _i32, _d, _i32, _i32]),
    "dv_field_set_fit_flux_groups": (C.c_int, [_p, C.c_int64, _d, _d, C.POINTER(DvFitFluxParams), _d, _d, _d, _d, _i32, _d, _i32,
                                               _i32, _i32]),
    "dv_infer_mc": (C.c_int, [_p, _f, C.c_int64, C.c_int32, C.c_uint64, _f, _f]),
    "dv_encode": (C.c_int, [_p, _f, C.c_int64, _f]),
    "dv_decode": (C.c_int, [_p, _f, C.c_int64, _f, _f]),
    "dv_model_get_activation": (C.c_int, [_p, C.c_char_p, _f, C.c_size_t]),
    "dv_prof_enable": (C.c_int, [_p, C.c_int32]),
    "dv_prof_read": (C.c_int, [_p, C.c_int32, _i64, C.POINTER(C.c_double)]),
    "dv_prof_reset": (C.c_int, [_p]),
    "dv_prof_read_family": (C.c_int, [_p, C.c_int32, C.c_char_p, C.c_size_t, _i64, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

def bind(handle, signatures):
    """restype / argtypes of every listed symbol on a loaded library (raises AttributeError for a missing export)."""
    for _name, (_res, _args) in signatures.items():
        _fn = getattr(handle, _name)
        _fn.restype = _res
        _fn.argtypes = _args
    return handle


bind(lib, SIGNATURES)
# dv_build_kind() == 1: a DEVELOPMENT build of the engine was selected with DEBVADER_AMD_LIB (it carries measurement
# switches that give wrong results and the one-GPU rehearsal hooks).  The package honours DV_DEBUG_SAME_GPU /
# DV_DEBUG_FAKE_PEERS only then; with the product library those variables do nothing.
IS_DEBUG_LIB = lib.dv_build_kind() == 1


def last_error() -> str:
    buf = C.create_string_buffer(512)
    lib.dv_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(status: int):
    if status != 0:
        raise DvError(status, last_error())
