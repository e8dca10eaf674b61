"""ctypes binding of libcpx_hip.so (include/cpx.h).  Loading never touches the
GPU; every compute call needs one and fails loudly otherwise."""

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CPX_LIB") or os.path.join(_HERE, "libcpx_hip.so")  # CPX_LIB: tuning builds only

CPX_OK = 0
STATUS = {
    0: "CPX_OK",
    -1: "CPX_ERR_INVALID",
    -2: "CPX_ERR_UNSUPPORTED",
    -3: "CPX_ERR_NO_DEVICE",
    -4: "CPX_ERR_HIP",
    -5: "CPX_ERR_OVERFLOW",
    -6: "CPX_ERR_NOMEM",
}


class CpxError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__("%s (%d) %s" % (STATUS.get(code, "CPX_ERR"), code, what))


class Config(C.Structure):
    _fields_ = [
        ("width", C.c_int32),
        ("height", C.c_int32),
        ("edge_pixels", C.c_int32),
        ("window", C.c_int32),
        ("background_thresh", C.c_double),
        ("weight_add", C.c_double),
        ("max_components", C.c_int32),
        ("max_frames", C.c_int32),
        ("denoise", C.c_int32),
        ("reserved", C.c_int32),
    ]


FRAME_META_DTYPE = np.dtype(
    [("time_on_ms", "<i8"), ("last_ffc_ms", "<i8"), ("background_frame", "<i4"), ("has_times", "<i4")]
)
COMPONENT_DTYPE = np.dtype(
    [("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"), ("area", "<i4"),
     ("sum_x", "<i4"), ("sum_y", "<i4"), ("pixel_variance", "<f4")]
)
FRAME_INFO_DTYPE = np.dtype(
    [("frame_number", "<i4"), ("n_components", "<i4"), ("status", "<i4"), ("ffc_affected", "<i4"),
     ("avg_change", "<i4"), ("norm_min", "<i4"), ("norm_max", "<i4"), ("threshold", "<f4"),
     ("filt_min", "<i4"), ("filt_max", "<i4"), ("thermal_min", "<i4"), ("thermal_max", "<i4"),
     ("thermal_sum", "<u4"), ("thermal_median", "<f4"), ("filtered_abs_sum", "<u8"),
     ("background_average", "<f8"), ("background_changed", "<i4"), ("reserved", "<i4")]
)
REGION_REF_DTYPE = np.dtype([("frame", "<i4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"),
                             ("in_segment", "<i4")])
TRACK_LIMITS_DTYPE = np.dtype([("filt_min", "<f4"), ("filt_max", "<f4"), ("clip_at_zero", "<i4"), ("flags", "<i4"),
                               ("therm_min", "<f4"), ("therm_max", "<f4"), ("reserved", "<i4", (2,))])
CROP_REQ_DTYPE = np.dtype([("frame", "<i4"), ("x", "<i4"), ("y", "<i4"), ("width", "<i4"), ("height", "<i4"),
                           ("track", "<i4"), ("sample", "<i4"), ("tile", "<i4")])
THUMB_STAT_DTYPE = np.dtype([("contours", "<i4"), ("status", "<i4"), ("median_diff", "<f8")])
CONV_TIMING_DTYPE = np.dtype([("key", "<i4"), ("launches", "<i4"), ("total_ms", "<f8"), ("flops", "<f8")])
# cpx_cptv_file / cpx_cptv_file_result / cpx_cptv_frame_slot (gzip inflate + section index on the device)
CPTV_FILE_DTYPE = np.dtype([("in_offset", "<i8"), ("in_bytes", "<i8"), ("out_offset", "<i8"), ("out_capacity", "<i8"),
                            ("slot_offset", "<i8"), ("slot_capacity", "<i4"), ("reserved", "<i4")])
CPTV_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_frames", "<i4"), ("out_bytes", "<i8"), ("in_consumed", "<i8"),
                              ("header_bytes", "<i4"), ("width", "<i4"), ("height", "<i4"), ("reserved", "<i4")])
CPTV_SLOT_DTYPE = np.dtype([("offset", "<i8"), ("bit_width", "<i4"), ("time_on_ms", "<u4"), ("last_ffc_ms", "<u4"),
                            ("temp_c", "<f4"), ("last_ffc_temp_c", "<f4"), ("flags", "<u4")])
CPTV_HEADER_BYTES = 1024
CPTV_BACKGROUND_FRAME, CPTV_HAS_TIME_ON, CPTV_HAS_LAST_FFC = 1, 2, 4
CPTV_STATUS = {1: "deflate: reserved block type", 2: "deflate: stored block length", 3: "deflate: block header",
               4: "deflate: code lengths", 5: "deflate: invalid symbol", 6: "deflate: distance too far back",
               7: "inflated data larger than the gzip trailer says", 8: "deflate: input exhausted (truncated file)",
               9: "deflate: no end-of-block code", 10: "not a gzip member", 11: "gzip trailer / further member", 12: "gzip CRC-32 mismatch",
               20: "not a CPTV file", 21: "unsupported CPTV version", 22: "CPTV header section", 23: "expected frame section",
               24: "truncated CPTV frame", 25: "malformed CPTV frame section", 26: "more frames than slots",
               27: "CPTV file has no frames"}
assert CPTV_FILE_DTYPE.itemsize == 48 and CPTV_RESULT_DTYPE.itemsize == 40 and CPTV_SLOT_DTYPE.itemsize == 32
assert REGION_REF_DTYPE.itemsize == 24 and TRACK_LIMITS_DTYPE.itemsize == 32 and CROP_REQ_DTYPE.itemsize == 32
assert FRAME_META_DTYPE.itemsize == 24 and COMPONENT_DTYPE.itemsize == 32 and FRAME_INFO_DTYPE.itemsize == 80

class WRResNetBlock(C.Structure):  # struct cpx_wrresnet_block
    _fields_ = [(k, C.c_void_p) for k in ("in_scale", "in_shift", "wa", "a_scale", "a_shift", "wb", "bb")]


class WRResNetParams(C.Structure):  # struct cpx_wrresnet_params
    _fields_ = [("n_labels", C.c_int32), ("blocks_per_stage", C.c_int32), ("groups", C.c_int32),
                ("in_channels", C.c_int32), ("filters", C.c_int32 * 4),
                ("conv1_w", C.c_void_p), ("conv1_b", C.c_void_p),
                ("block", (WRResNetBlock * 8) * 3),
                ("shortcut_w", C.c_void_p * 3), ("shortcut_b", C.c_void_p * 3),
                ("final_scale", C.c_void_p), ("final_shift", C.c_void_p),
                ("dense_w", C.c_void_p), ("dense_b", C.c_void_p),
                ("n_hidden", C.c_int32), ("activation", C.c_int32), ("hidden_sizes", C.c_int32 * 4),
                ("hidden_w", C.c_void_p * 4), ("hidden_b", C.c_void_p * 4)]


class HeadDesc(C.Structure):  # struct cpx_head_desc
    _fields_ = [("N", C.c_int32), ("HW", C.c_int32), ("C", C.c_int32), ("L", C.c_int32),
                ("n_hidden", C.c_int32), ("activation", C.c_int32), ("hidden_sizes", C.c_int32 * 4),
                ("in_dev", C.c_void_p), ("bn_scale_dev", C.c_void_p), ("bn_shift_dev", C.c_void_p),
                ("hidden_w_dev", C.c_void_p * 4), ("hidden_b_dev", C.c_void_p * 4),
                ("dense_w_dev", C.c_void_p), ("dense_b_dev", C.c_void_p),
                ("logits_dev", C.c_void_p), ("probs_dev", C.c_void_p)]


class GraphTensor(C.Structure):  # struct cpx_graph_tensor
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32), ("c_offset", C.c_int32), ("c_stride", C.c_int32),
                ("type", C.c_int32), ("arena_offset", C.c_int64)]


class GraphOp(C.Structure):  # struct cpx_graph_op
    _fields_ = [("kind", C.c_int32), ("in0", C.c_int32), ("in1", C.c_int32), ("out", C.c_int32),
                ("kh", C.c_int32), ("kw", C.c_int32), ("stride_h", C.c_int32), ("stride_w", C.c_int32),
                ("pad_top", C.c_int32), ("pad_left", C.c_int32), ("pad_bottom", C.c_int32), ("pad_right", C.c_int32),
                ("activation", C.c_int32), ("out_c_offset", C.c_int32), ("out_c_stride", C.c_int32),
                ("n_map", C.c_int32), ("channel_map", C.c_int32 * 4), ("param", C.c_float),
                ("weights", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p)]


assert C.sizeof(WRResNetParams) == 1560
assert C.sizeof(GraphTensor) == 32 and C.sizeof(GraphOp) == 112
# enum CPX_GRAPH_* (include/cpx.h)
GRAPH_CONV, GRAPH_MAX_POOL, GRAPH_AVG_POOL, GRAPH_ADD, GRAPH_AFFINE, GRAPH_MEAN, GRAPH_FC, GRAPH_LOGISTIC, GRAPH_SOFTMAX, \
    GRAPH_PAD, GRAPH_CHANNEL_MAP, GRAPH_CONV_Q8, GRAPH_FC_Q8, GRAPH_QUANT_PARAMS, GRAPH_DWCONV, GRAPH_DWCONV_Q8, GRAPH_MUL, \
    GRAPH_INPUT, GRAPH_CONV_PRE, GRAPH_SLICE, GRAPH_DWCONV_PRE, GRAPH_RANGE, GRAPH_CONV_F16X2, GRAPH_CONV_GROUPED, \
    GRAPH_CONV_Q8_GROUPED = range(1, 26)
# the full-integer operators (int8 activations); enum CPX_GRAPH_TYPE_* and CPX_GRAPH_I8_HDR_*
GRAPH_QUANTIZE, GRAPH_DEQUANTIZE, GRAPH_CONV_I8, GRAPH_CONV_I8_GROUPED, GRAPH_DWCONV_I8, GRAPH_FC_I8, GRAPH_ADD_I8, \
    GRAPH_MUL_I8, GRAPH_MAX_POOL_I8, GRAPH_AVG_POOL_I8, GRAPH_MEAN_I8, GRAPH_LUT_I8 = range(26, 38)
GRAPH_TYPE_FLOAT32, GRAPH_TYPE_INT8 = 0, 1
GRAPH_I8_HDR_Z_IN, GRAPH_I8_HDR_Z_IN1, GRAPH_I8_HDR_Z_OUT, GRAPH_I8_HDR_LO, GRAPH_I8_HDR_HI, GRAPH_I8_HDR_M0, GRAPH_I8_HDR_S0, \
    GRAPH_I8_HDR_M1, GRAPH_I8_HDR_S1, GRAPH_I8_HDR_MO, GRAPH_I8_HDR_SO, GRAPH_I8_HDR_LEFT = range(12)
GRAPH_I8_HDR_WORDS = 16
GRAPH_I8_LUT_BYTES = 4 * GRAPH_I8_HDR_WORDS + 256   # the header with a 256-entry int8 table behind it (LUT_I8, ACT_LUT)
# enum CPX_GRAPH_ACT_*: the planner's own activation codes, outside TFLite's ActivationFunctionType
GRAPH_ACT_SWISH, GRAPH_ACT_LOGISTIC, GRAPH_ACT_LUT = 16, 17, 18
GRAPH_MEAN_WIDE_PIXELS = 256   # MEAN: from this many pixels on the striped summation order (csrc/cpx_graph_core.h)
GRAPH_CONV_KC, GRAPH_CONV_CO = 16, 32   # CONV weights: Cin / Cout rounded up to these (csrc/cpx_kernels.h)
GRAPH_CONV_Q8_KC = 32   # CONV_Q8 weights: int8 in MFMA fragment order, Cin rounded up to this (csrc/cpx_kernels.h)
GRAPH_CONV_H2_KC = 32   # CONV_F16X2 weights: two fp16 planes in MFMA fragment order, Cin rounded up to this (csrc/cpx_kernels.h)
HEAD_SIGMOID, HEAD_SOFTMAX = 0, 1


# One entry per function of include/cpx.h: name -> (restype, [argtypes]).  load() declares the prototypes from it, call() and
# status() marshal by it, tests/test_binding_cpu.py holds it against the header.
def _signatures():
    i, vp = C.c_int, C.c_void_p
    i32p, intp, f32p, vpp, sizep = (C.POINTER(ty) for ty in (C.c_int32, C.c_int, C.c_float, C.c_void_p, C.c_size_t))
    return {
        "cpx_abi_version": (i, []),
        "cpx_create": (i, [i, C.POINTER(Config), vpp]),
        "cpx_destroy": (None, [vp]),
        "cpx_last_error": (C.c_char_p, [vp]),
        "cpx_stream": (vp, [vp]),
        "cpx_synchronize": (i, [vp]),
        "cpx_join_medians": (i, [vp]),
        "cpx_release_memory": (i, [vp]),
        "cpx_track_batch": (i, [vp, vp, i32p, vp, i, vp, vp, vp, vp, vp]),
        "cpx_track_workspace_bytes": (C.c_size_t, [vp, i, i]),
        "cpx_last_kernel_timing": (i, [vp, f32p, intp]),
        "cpx_associate_batch": (i, [vp, vp, i32p, vp, i, vp, vp, vp, vp, vp, vp, vp, vp]),
        "cpx_track_limits_batch": (i, [vp, vp, vp, vp, vp, vp, i, vp]),
        "cpx_crop_tile": (i, [vp, vp, vp, vp, vp, i, vp, i, i, vp]),
        "cpx_conv2d": (i, [vp, vp]),
        "cpx_cnn_head": (i, [vp, vp, i, i, i, vp, vp, vp, vp, i, vp, vp]),
        "cpx_finalize_tracks": (i, [vp, vp, i32p, vp, i, vp, vp, vp, vp, vp]),
        "cpx_counts_prefix": (i, [vp, vp, i, vp]),
        "cpx_plan_segments": (i, [vp, vp, i32p, vp, i, vp, vp, vp, vp, i, vp, vp, vp, vp, vp]),
        "cpx_aggregate_predictions": (i, [vp, vp, vp, i, vp, i, i, i, i, vp, vp]),
        "cpx_conv_timing_enable": (i, [vp, i]),
        "cpx_conv_timing_report": (i, [vp, vp, i, intp]),
        "cpx_cptv_unpack": (i, [vp, vp, vp, vp, vp, i, vp]),
        "cpx_thumb_stats": (i, [vp, vp, vp, vp, vp, i, vp]),
        "cpx_trackless_thumb": (i, [vp, vp, i, i, vp]),
        "cpx_trackless_thumb_batch": (i, [vp, vp, vp, i, vp]),
        "cpx_thumb_stats_ex": (i, [vp, vp, vp, vp, vp, i, vp, i, i, i]),
        "cpx_track_frame": (i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp]),
        "cpx_associate_frame": (i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp]),
        "cpx_cnn_create": (i, [vp, C.POINTER(WRResNetParams), vpp]),
        "cpx_cnn_destroy": (None, [vp]),
        "cpx_cnn_forward": (i, [vp, vp, i, i, i, vp, vp]),
        "cpx_ir_detect": (i, [vp, vp, i, i, i, i, i, vp, vp, vp, vp]),
        "cpx_set_cnn_math": (i, [vp, i]),
        "cpx_get_cnn_math": (i, [vp]),
        "cpx_mog2_create": (i, [vp, i, i, i, i, C.c_float, vpp]),
        "cpx_mog2_apply": (i, [vp, vp, C.c_double, vp]),
        "cpx_mog2_background": (i, [vp, vp]),
        "cpx_mog2_destroy": (None, [vp]),
        "cpx_track_batch_ex": (i, [vp, vp, i32p, vp, i, vp, vp, vp, vp, vp, i]),
        "cpx_track_frame_ex": (i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, i]),
        "cpx_set_background": (i, [vp, i, vp, vp, C.c_double]),
        "cpx_get_background": (i, [vp, i, vp, vp, C.POINTER(C.c_double)]),
        "cpx_track_limits_batch_ex": (i, [vp, vp, vp, vp, vp, vp, i, vp, i]),
        "cpx_cnn_head_ex": (i, [vp, C.POINTER(HeadDesc)]),
        "cpx_ir_delta_variance": (i, [vp, vp, vp, i, i, vp, i, vp]),
        "cpx_cptv_inflate": (i, [vp, vp, vp, i, vp, vp, vp, vp]),
        "cpx_cptv_gather_index": (i, [vp, vp, vp, vp, i, vp, vp, vp]),
        "cpx_format_regions": (C.c_long, [vp, i, C.c_long, i, i, i, vp, C.c_long]),
        "cpx_json_indent": (C.c_long, [C.c_char_p, C.c_long, i, i, vp, C.c_long]),
        "cpx_ir_merge": (i, [vp, vp, vp, i, i, i, vp, vp, i, i, i, i, vp, vp, vp]),
        "cpx_ir_resize_area": (i, [vp, vp, i, i, i, i, vp]),
        "cpx_ir_frame_statistics": (i, [vp, vp, vp, i, i, vp, vp]),
        "cpx_cnn_last_overflow": (i, [vp, intp]),
        "cpx_cnn_set_activation_bounds": (i, [vp, f32p, i]),
        "cpx_cnn_overflow_forwards": (i, [vp, intp, i]),
        "cpx_cnn_forward_taps": (i, [vp, vp, i, i, i, vp, vp, vpp, i, vp]),
        "cpx_graph_create": (i, [vp, C.POINTER(GraphOp), i, C.POINTER(GraphTensor), i, i, i, vpp]),
        "cpx_graph_forward": (i, [vp, vp, i, vp]),
        "cpx_graph_arena_bytes": (i, [vp, i, sizep]),
        "cpx_graph_arena_allocated": (i, [vp, sizep]),
        "cpx_graph_destroy": (None, [vp]),
        "cpx_cnn_set_residual_bounds": (i, [vp, f32p, i]),
        "cpx_cnn_shortcut_scale": (i, [C.c_float, C.c_float, f32p]),
    }


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)

IR_FRAME_STATS_DTYPE = np.dtype([("min", "<i4"), ("max", "<i4"), ("sum", "<i8"), ("median_x2", "<i4"), ("reserved", "<i4"),
                                 ("filtered_sum", "<i8")])
assert IR_FRAME_STATS_DTYPE.itemsize == 32

# flags of cpx_track_batch_ex / cpx_track_frame_ex and cpx_track_limits_batch_ex (include/cpx.h)
TRACK_KEEP_BACKGROUND, TRACK_FREEZE_ON_FFC, TRACK_FREEZE_BACKGROUND, TRACK_DEFER_MEDIANS = 1, 2, 4, 8
LIMITS_POST_PROCESS, LIMITS_THERMAL_DIFF_NORM, LIMITS_NO_DIFF_NORM, LIMITS_ALWAYS_CLIP, LIMITS_SWAP_CHANNELS = 1, 2, 4, 8, 16
LIMITS_TF_SCALING = 32

_lib = None


def load():
    """dlopen the library and declare the prototypes.  Raises if it is missing:
    there is no CPU fallback for the compute path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libcpx_hip.so not built: run `python __graft_entry__.py` (or make -C classifier-pipeline_amd/csrc)")
    # PyTorch-ROCm bundles its own libamdhip64; it must be the HIP runtime of the
    # process (two runtimes cannot share the device), so load torch before us.
    try:
        import torch  # noqa: F401
    except ImportError:  # pure ctypes use without torch: the system runtime is fine
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        declare(getattr(lib, name), restype, argtypes)
    if lib.cpx_abi_version() != 3:
        raise ImportError("libcpx_hip.so ABI version mismatch")
    _lib = lib
    return lib


def ptr(x, what="a cpx call"):
    """What a call site holds -> what ctypes takes for a pointer parameter: None -> NULL, a torch tensor -> its
    data_ptr(), a numpy array -> its ctypes.data, a ctypes Structure -> byref; ctypes pointers, byref objects, ints,
    floats and bytes pass through.  The kernels index densely, so a tensor or array that is not contiguous is refused."""
    if x is None or type(x) is C.c_void_p:   # (the two cheapest first: this runs per argument of every call)
        return x
    data_ptr = getattr(x, "data_ptr", None)
    if data_ptr is not None:
        if not x.is_contiguous():
            raise ValueError("%s: tensor of shape %s, strides %s is not contiguous" % (what, tuple(x.shape), x.stride()))
        return C.c_void_p(data_ptr())
    if isinstance(x, np.ndarray):
        if not x.flags.c_contiguous:
            raise ValueError("%s: array of shape %s, strides %s is not C-contiguous" % (what, x.shape, x.strides))
        return C.c_void_p(x.ctypes.data)
    if isinstance(x, C.Structure):
        return C.byref(x)
    return x


def declare(fn, restype, argtypes):
    """Give a function of the library its entry of the table: the prototype ctypes converts by, and -- worked out here,
    once, not per call -- how many parameters it takes and where the pointers among them stand: fn.pointers = ((position,
    the POINTER type an address is cast to, or None for void * / char *), ...).  Both live on the function object that
    load() fetched (the one `lib.<name>` hands out from then on): status() takes no other."""
    fn.restype, fn.argtypes, fn.arity = restype, argtypes, len(argtypes)
    fn.pointers = tuple((k, None if ty in (C.c_void_p, C.c_char_p) else ty) for k, ty in enumerate(argtypes)
                        if ty in (C.c_void_p, C.c_char_p) or issubclass(ty, C._Pointer))


def status(lib, name, *args):
    """lib.<name>(...) with ptr() applied to every argument the function declares as a pointer -> its integer status."""
    fn = getattr(lib, name)
    try:
        pointers = fn.pointers
    except AttributeError:
        raise TypeError("%s has no declared prototype: take the library from cpx._lib.load()" % name) from None
    if len(args) != fn.arity:
        raise TypeError("%s takes %d arguments, %d given" % (name, fn.arity, len(args)))
    args = list(args)
    for k, typed in pointers:
        a = ptr(args[k], name)
        if typed is not None and type(a) is C.c_void_p:   # an address for a typed pointer (int32_t *clip_offsets)
            a = C.cast(a, typed)
        args[k] = a
    return fn(*args)


def check(lib, err_handle, rc):
    """Raise CpxError with cpx_last_error(err_handle) as its text when the status rc is not CPX_OK."""
    if rc != 0:
        raise CpxError(rc, (lib.cpx_last_error(err_handle) or b"").decode())


def call(lib, err_handle, name, *args):
    """status(), checked."""
    check(lib, err_handle, status(lib, name, *args))
