"""The op list ABI of libcrossloc_hip (include/crossloc_cnn.h): op and flag constants, the `xl_op` structure, the ctypes
binding of the CNN entry points and their status check."""
import ctypes

import numpy as _np

from . import _lib

XL_OP_CONV1, XL_OP_CONV, XL_OP_GN_STATS, XL_OP_GN_APPLY, XL_OP_HEAD = 0, 1, 2, 3, 4
GN_RELU_IN, GN_ADD, GN_RELU_OUT, GN_ACC_AUX, GN_NO_CONV_BIAS = 1, 2, 4, 8, 16
XL_OP_WGRAD, XL_OP_GNB_STATS, XL_OP_GNB_APPLY, XL_OP_GNB_PARAMS, XL_OP_HEAD_BWD, XL_OP_CONV1_WGRAD = 5, 6, 7, 8, 9, 10
XL_OP_GN_FINAL = 11
XL_OP_WINO_IN, XL_OP_WINO_OUT = 12, 13
XL_OP_DUC_HEAD = 14
XL_OP_DUC_HEAD_BWD = 15
XL_OP_WINO_DY, XL_OP_WINO_WFINAL, XL_OP_GNB_FINAL = 16, 17, 18
XL_OP_STEM12 = 19
XL_OP_S2_DGRAD = 20
CONV_DGRAD, CONV_ACCUMULATE, CONV_SPLIT_BF16 = 1, 2, 64
CONV_NORM_IN, CONV_NORM_RELU = 128, 256
CONV_SPLIT_IL = 512
CONV_SPLIT_ACT = 1024
CONV_M_TILE_MAJOR = 2048
CONV_NORM_ADD = 4096
CONV_PAIR_F16 = 8192
CONV_PAIR_AMAX = 16384
XL_OP_FILL0 = 21
XL_OP_GNB_PARAMS_LIST = 22
# entries of the device tables of xl_cnn_repack_pairs / XL_OP_GNB_PARAMS_LIST (include/crossloc_cnn.h: xl_pair_item, xl_gnb_params_item)

PAIR_ITEM_DTYPE = _np.dtype([("src", "<u8"), ("dst", "<u8"), ("rows", "<i4"), ("K", "<i4"), ("kind", "<i4"), ("pad", "<i4")])
GNB_PARAMS_ITEM_DTYPE = _np.dtype([("sums", "<u8"), ("gamma", "<u8"), ("dgamma", "<u8"), ("dbeta", "<u8"), ("dbias", "<u8"),
                                   ("B", "<i4"), ("C", "<i4"), ("G", "<i4"), ("HW", "<i4")])
XL_ERR_UNSUPPORTED = -4            # include/crossloc_dsac.h


class XlOp(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in
                ("type", "B", "Hi", "Wi", "Cin", "Ho", "Wo", "Cout", "ksize", "stride", "groups", "nchunks",
                 "flags", "ld_in", "ld_out", "ld_aux", "n_task", "n_pos", "nchunks2", "reserved_i")] + \
               [(n, ctypes.c_float) for n in ("eps", "clamp_lo", "clamp_hi", "reserved")] + \
               [(n, ctypes.c_void_p) for n in ("in_", "w", "bias", "aux", "stats", "out", "aux2", "out2", "stats2", "scale")]


def _bind():
    L = _lib.lib()
    if not hasattr(L, "_cnn_bound"):
        L.xl_cnn_run.restype = ctypes.c_int
        L.xl_cnn_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.xl_cnn_op_size.restype = ctypes.c_int
        L.xl_cnn_pack_conv_weight.restype = ctypes.c_int
        L.xl_cnn_pack_conv_weight.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_void_p]
        L.xl_cnn_pack_conv_weight_dgrad.restype = ctypes.c_int
        L.xl_cnn_pack_conv_weight_dgrad.argtypes = L.xl_cnn_pack_conv_weight.argtypes
        L.xl_cnn_pack_wino_weight.restype = ctypes.c_int
        L.xl_cnn_pack_wino_weight.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
        L.xl_cnn_split_weight.restype = ctypes.c_int
        L.xl_cnn_split_weight.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.xl_cnn_pack_wino_weight_pair.restype = ctypes.c_int
        L.xl_cnn_pack_wino_weight_pair.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
        L.xl_cnn_pair_weight.restype = ctypes.c_int
        L.xl_cnn_pair_weight.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.xl_cnn_repack_pairs.restype = ctypes.c_int
        L.xl_cnn_repack_pairs.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p]
        L.xl_cnn_pair_activation.restype = ctypes.c_int
        L.xl_cnn_pair_activation.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.xl_cnn_pair_scales.restype = ctypes.c_int
        L.xl_cnn_pair_scales.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p]
        L.xl_cnn_graph_capture.restype = ctypes.c_int
        L.xl_cnn_graph_capture.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        L.xl_cnn_graph_launch.restype = ctypes.c_int
        L.xl_cnn_graph_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.xl_cnn_graph_destroy.restype = ctypes.c_int
        L.xl_cnn_graph_destroy.argtypes = [ctypes.c_void_p]
        L.xl_cnn_last_error.restype = ctypes.c_char_p
        L.xl_cnn_item_size.restype = ctypes.c_int
        L.xl_cnn_item_size.argtypes = [ctypes.c_int]
        if (L.xl_cnn_item_size(0), L.xl_cnn_item_size(1)) != (PAIR_ITEM_DTYPE.itemsize, GNB_PARAMS_ITEM_DTYPE.itemsize):
            raise _lib.XlError("device-table entry layout mismatch: C %d / %d vs numpy %d / %d" % (
                L.xl_cnn_item_size(0), L.xl_cnn_item_size(1), PAIR_ITEM_DTYPE.itemsize, GNB_PARAMS_ITEM_DTYPE.itemsize))
        if L.xl_cnn_op_size() != ctypes.sizeof(XlOp):
            raise _lib.XlError("xl_op layout mismatch: C %d vs ctypes %d" % (L.xl_cnn_op_size(), ctypes.sizeof(XlOp)))
        L._cnn_bound = True
    return L


def _check(rc):
    if rc != 0:
        L = _lib.lib()
        raise _lib.XlError("crossloc_hip cnn: %s %s (status %d)" % (
            L.xl_status_string(rc).decode(), L.xl_cnn_last_error().decode(), rc))


def act_ptr(act):
    """Byte address of an activation tuple (tensor, H, W, C, ld, channel offset): fp32, NHWC, `off` channels in."""
    return act[0].data_ptr() + 4 * act[5]
