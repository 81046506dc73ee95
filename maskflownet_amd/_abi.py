"""ctypes signatures of the C ABI declared in include/mfn_hip.h.

`bind(cdll, prefix)` attaches argtypes/restype to every entry point and returns a namespace
whose attributes are the functions without the prefix.  The product binds libmfn_hip.so with
prefix "mfn_"; tests bind the kernel-logic emulation build with prefix "mfn_emu_".
"""
import ctypes as C
from types import SimpleNamespace

_f = C.c_void_p      # const float* / float*  (device or host address as integer)
_i = C.c_int
_s = C.c_void_p      # hipStream_t
_pi = C.POINTER(C.c_int)

SIGNATURES = {
    # name: (restype, [argtypes])
    "last_error": (C.c_char_p, []),
    "correlation_out_shape": (_i, [_i] * 7 + [_pi, _pi, _pi]),
    "correlation_fwd": (_i, [_f, _f, _f] + [_i] * 10 + [_s]),
    "correlation_workspace_bytes": (C.c_size_t, [_i] * 10),
    "correlation_fwd_ws": (_i, [_f, _f, _f] + [_i] * 10 + [C.c_void_p, C.c_size_t, _s]),
    "correlation_fwd_act": (_i, [_f, _f, _f] + [_i] * 11 + [C.c_void_p, C.c_size_t, _s]),
    "correlation_fwd_into": (_i, [_f, _f, _f, C.c_longlong] + [_i] * 11 + [C.c_void_p, C.c_size_t, _s]),
    "warp_fwd": (_i, [_f, _f, _f] + [_i] * 5 + [_s]),
    "grid_generator_warp": (_i, [_f, _f, _i, _i, _i, _s]),
    "grid_generator_affine": (_i, [_f, _f, _i, _i, _i, _s]),
    "bilinear_sampler_fwd": (_i, [_f, _f, _f] + [_i] * 6 + [_s]),
    "bilinear_sampler_bwd": (_i, [_f] * 5 + [_i] * 8 + [_s]),
    "grid_generator_warp_bwd": (_i, [_f, _f] + [_i] * 4 + [_s]),
    "deform_conv_out_shape": (_i, [_i] * 10 + [_pi, _pi]),
    "deform_conv_workspace_bytes": (C.c_size_t, [_i] * 15),
    "deform_conv_fwd": (_i, [_f] * 5 + [_i] * 15 + [C.c_void_p, C.c_size_t, _s]),
    "deform_conv_shared_fwd": (_i, [_f, _f, C.c_float, C.c_float, _f, _f, _f] + [_i] * 12 + [C.c_void_p, C.c_size_t, _s]),
    "offsets_from_flow": (_i, [_f, _f, _i, _i, _i, _i, C.c_float, C.c_float, _s]),
    "offsets_from_flow_bwd": (_i, [_f, _f, _i, _i, _i, _i, C.c_float, C.c_float, _i, _s]),
    "deform_conv_shared_bwd_workspace_bytes": (C.c_size_t, [_i] * 12),
    "deform_conv_shared_bwd": (_i, [_f, _f, _f, C.c_float, C.c_float, _f, _f, _f, _f, _f] + [_i] * 16 + [C.c_void_p, C.c_size_t, _s]),
    "debug_set_timeline": (_i, [C.c_void_p]),
    "debug_last_dc_plan": (_i, [_pi, _pi, _pi, _pi]),
    "correlation_bwd": (_i, [_f] * 5 + [_i] * 12 + [_s]),
    "warp_bwd": (_i, [_f] * 5 + [_i] * 7 + [_s]),
    "deform_conv_packed_weight_bytes": (C.c_size_t, [_i] * 15),
    "deform_conv_pack_weights": (_i, [_f] + [_i] * 15 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_ulonglong), _s]),
    "deform_conv_fwd_packed": (_i, [_f, _f, C.c_void_p, C.c_size_t, C.c_ulonglong, _f, _f] + [_i] * 15 + [C.c_void_p, C.c_size_t, _s]),
    "deform_conv_shared_fwd_packed": (_i, [_f, _f, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_ulonglong, _f, _f] + [_i] * 12 + [C.c_void_p, C.c_size_t, _s]),
    "upsample_fwd": (_i, [_f, _f] + [_i] * 5 + [_s]),
    "deform_conv_matching_fwd": (_i, [_f, _f, C.c_float, C.c_float, _f, C.c_void_p, C.c_size_t, C.c_ulonglong, _f, _f, _f, _i, _f]
                                 + [_i] * 12 + [C.c_void_p, C.c_size_t, _s]),
    "deform_conv_bwd_workspace_bytes": (C.c_size_t, [_i] * 15),
    "deform_conv_bwd": (_i, [_f] * 8 + [_i] * 19 + [C.c_void_p, C.c_size_t, _s]),
    "conv2d_out_shape": (_i, [_i] * 13 + [_pi, _pi]),
    "conv2d_workspace_bytes": (C.c_size_t, [_i] * 15),
    "conv2d_packed_weight_bytes": (C.c_size_t, [_i] * 15),
    "conv2d_pack_weights": (_i, [_f] + [_i] * 15 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_ulonglong), _s]),
    "conv2d_fwd": (_i, [_f, C.c_longlong, _f, C.c_void_p, C.c_size_t, C.c_ulonglong, _f, _f, C.c_longlong] + [_i] * 18 + [C.c_void_p, C.c_size_t, _s]),
    "upsample_bwd": (_i, [_f, _f] + [_i] * 6 + [_s]),
    "leaky_relu_bwd": (_i, [_f, _f, _f, C.c_size_t, C.c_float, _s]),
    # the matching module's gate on its own, forward and backward (kernels/gate.h)
    "matching_gate_fwd": (_i, [_f, _f, _f, _i, _f] + [_i] * 4 + [_s]),
    "matching_gate_bwd_workspace_bytes": (C.c_size_t, [_i] * 4),
    "matching_gate_bwd": (_i, [_f] * 5 + [_i] + [_f] * 3 + [_i] * 7 + [C.c_void_p, C.c_size_t, _s]),
    "conv2d_bwd_workspace_bytes": (C.c_size_t, [_i] * 18),
    "conv2d_bwd": (_i, [_f] * 7 + [_i] * 21 + [C.c_void_p, C.c_size_t, _s]),
    # augmentation of the training batch (kernels/augment.h); bound by the emulation build as well
    "augment_geometry": (_i, [_f, _f, _f, _f, _i, _f, _f, _f, _f, _f] + [_i] * 6 + [_s]),
    "augment_color_mean_workspace_bytes": (C.c_size_t, [_i] * 3),
    "augment_color_mean": (_i, [_f, _f, _f, C.c_float, C.c_ulonglong, C.c_ulonglong, _f] + [_i] * 3 + [C.c_void_p, C.c_size_t, _s]),
    "augment_color": (_i, [_f, _f, _f, _f, C.c_float, C.c_ulonglong, C.c_ulonglong, _i, _i, _f] + [_i] * 3 + [_s]),
    # the fused multiscale training loss (kernels/loss.h); host arrays of pointers / ints / floats
    "multiscale_epe_workspace_bytes": (C.c_size_t, [_i] * 4),
    "multiscale_epe_fwd": (_i, [C.POINTER(C.c_void_p), _pi, C.POINTER(C.c_float), _i, _f, _f, _i, C.c_float, _i, C.c_float, _f, _f]
                           + [_i] * 3 + [C.c_void_p, C.c_size_t, _s]),
    "multiscale_epe_bwd": (_i, [_f, C.POINTER(C.c_void_p), _pi, C.POINTER(C.c_float), _i, _f, _f, _i, C.c_float, _i, C.c_float, _f,
                                C.POINTER(C.c_void_p), _pi] + [_i] * 3 + [_s]),
    # the trainer's Adam step (kernels/optimizer.h); the table entries are host-only
    "adam_update": (_i, [_f] * 4 + [C.c_longlong] + [C.c_float] * 7 + [_s]),
    "multi_adam_table_bytes": (C.c_size_t, [_i, C.POINTER(C.c_longlong)]),
    "multi_adam_build_table": (_i, [_i] + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(C.c_longlong), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.c_void_p, C.c_size_t, _pi, C.POINTER(C.c_ulonglong)]),
    "multi_adam_update": (_i, [C.c_void_p, C.c_size_t, C.c_ulonglong, _i, _i] + [C.c_float] * 7 + [_s]),
    # one training batch out of a device-resident data set (kernels/batch.h); the rows entries are host-only
    "batch_gather_rows_bytes": (C.c_size_t, [_i]),
    "batch_gather_build_rows": (_i, [_i] + [C.POINTER(C.c_void_p)] * 4 + [_pi] * 6 + [_i, _i, C.c_void_p, C.c_size_t, C.POINTER(C.c_ulonglong)]),
    "batch_gather": (_i, [C.c_void_p, C.c_size_t, C.c_ulonglong] + [_i] * 4 + [C.c_void_p] * 4 + [_s]),
    # a validation batch read through the rows of a resident data set (kernels/validate.h)
    "val_pair_mean_workspace_bytes": (C.c_size_t, [_i] * 3),
    "val_pair_mean": (_i, [C.c_void_p] + [_i] * 3 + [_f, C.c_void_p, C.c_size_t, _s]),
    "val_preprocess": (_i, [C.c_void_p] + [_i] * 3 + [_f, _f, _i, _i, _s]),
    "val_flow_metrics_workspace_bytes": (C.c_size_t, [_i] * 3),
    "val_flow_metrics": (_i, [C.c_void_p, _f] + [_i] * 3 + [_f, C.c_void_p, C.c_size_t, _s]),
    # raw decoded arrays into stored samples (kernels/ingest.h); the tables entries and png_unfilter are host-only
    "ingest_tables_bytes": (C.c_size_t, [_i, _i]),
    "ingest_build_tables": (_i, [_i] * 4 + [C.c_void_p, C.c_size_t, C.POINTER(C.c_ulonglong)]),
    "ingest_minmax": (_i, [C.c_void_p, C.c_void_p, _i, _i, C.c_longlong] + [_i] * 4 + [C.c_void_p, _s]),
    "ingest_image": (_i, [C.c_void_p, _i, _i, C.c_longlong] + [_i] * 4 + [C.c_void_p, C.c_size_t, C.c_ulonglong, _i, C.c_void_p, C.c_void_p, _i, _i, _s]),
    "ingest_flow_occ": (_i, [C.c_void_p, _i, _i, C.c_longlong] + [_i] * 4 + [C.c_void_p, C.c_size_t, C.c_ulonglong, _i, _i, C.c_void_p, C.c_void_p, _i, _i, _s]),
    "png_unfilter": (_i, [C.c_void_p, C.c_longlong, C.c_longlong, _i]),
    "set_arithmetic": (_i, [C.c_char_p, _i]),
    "get_arithmetic": (_i, [C.c_char_p, _pi]),
    "set_tuning": (_i, [C.c_char_p, _i]),
    "get_tuning": (_i, [C.c_char_p, _pi]),
}

# entry points that only the product library exports (HIP runtime plumbing, backward)
PRODUCT_ONLY = {
    "abi_version": (_i, []),
    "version_string": (C.c_char_p, []),
    "graph_begin_capture": (_i, [_s]),
    "graph_end_capture": (_i, [_s, C.POINTER(C.c_void_p)]),
    "graph_launch": (_i, [C.c_void_p, _s]),
    "graph_destroy": (_i, [C.c_void_p]),
    "profile_enable": (_i, [_i]),
    "profile_reset": (_i, []),
    "profile_tag": (_i, [C.c_char_p]),
    "profile_query": (_i, [C.c_char_p, _pi, C.POINTER(C.c_double)]),
    "profile_dump": (_i, [C.c_char_p, _i]),
    # prediction on images of any size (kernels/predict.h): the oracle has no twin of these, so the emulation build binds none
    "pair_mean_workspace_bytes": (C.c_size_t, [_i] * 4),
    "pair_mean": (_i, [_f, _f, _f] + [_i] * 4 + [C.c_void_p, C.c_size_t, _s]),
    "preprocess_pair": (_i, [_f, _f, _f, _f] + [_i] * 6 + [_s]),
    "bilinear_resize_fwd": (_i, [_f, _f, _f] + [_i] * 7 + [_s]),
    "flow_metrics_workspace_bytes": (C.c_size_t, [_i] * 3),
    "flow_metrics": (_i, [_f, _f, _f, _f] + [_i] * 3 + [C.c_void_p, C.c_size_t, _s]),
    # prediction on uint8 frame sequences, the colour picture of a flow (kernels/frames.h): product only, like the entries above
    "pair_mean_u8_workspace_bytes": (C.c_size_t, [_i] * 3),
    "pair_mean_u8": (_i, [C.c_void_p] + [_i] * 6 + [_f, C.c_void_p, C.c_size_t, _s]),
    "preprocess_pair_u8": (_i, [C.c_void_p] + [_i] * 6 + [_f, _f, _i, _i, _s]),
    "flow_color_workspace_bytes": (C.c_size_t, [_i] * 3),
    "flow_color": (_i, [_f, C.c_void_p, _i, _i, _i, C.c_float, _i, C.c_void_p, C.c_size_t, _s]),
}


def bind(cdll, prefix="mfn_", product=True):
    ns = SimpleNamespace()
    table = dict(SIGNATURES)
    if product:
        table.update(PRODUCT_ONLY)
    for name, (res, args) in table.items():
        fn = getattr(cdll, prefix + name)  # AttributeError = missing export
        fn.restype = res
        fn.argtypes = args
        setattr(ns, name, fn)
    ns._cdll = cdll
    return ns


def exported_names(product=True):
    names = list(SIGNATURES)
    if product:
        names += list(PRODUCT_ONLY)
    return names
