"""The refusals of the CNN launchers, forward and backward, as a table.  No GPU.

A launcher validates an op before it makes any HIP call and answers a malformed one with XL_ERR_ARG (-1) or XL_ERR_UNSUPPORTED
(-4); xl_cnn_run then names the op ("op 0 refused (...)") behind whatever text the launcher left.  Every row below is one
malformed op fed to xl_cnn_run alone, with null or dummy pointers (never dereferenced on the host) and stream = NULL, and
pins the exact status - for a handful also a piece of xl_cnn_last_error().  There is one row per refusing statement of the
launchers of XL_OP_CONV1, XL_OP_CONV (the fp32 implicit GEMM: dispatch and launcher), XL_OP_WINO_IN / XL_OP_WINO_OUT (m = 2,
4, 6), XL_OP_GN_STATS / GN_APPLY / GN_FINAL, XL_OP_HEAD and XL_OP_DUC_HEAD that is reached before the first HIP call, and rows
with two faults that pin which check comes first where the statuses differ.  The expected values were recorded from the
library before the launchers were split over translation units.  The same for the stride-2 3x3 stem convolutions
(XL_OP_CONV with XL_CONV_SPLIT_BF16, with and without XL_CONV_PAIR_F16) and the weight-gradient products on the matrix pipe
(XL_OP_WGRAD with XL_CONV_SPLIT_BF16, with and without XL_CONV_PAIR_F16, one split and several): one row per clause of their
refusing statements, recorded from the library while each operand form still had a launcher of its own.  And the same, one
row per clause, for the 1x1 / XL_CONV_SPLIT_ACT GEMMs of both operand forms (_g1_rows), the persistent batched GEMMs
(_gb_rows) and every backward op (_bwd_rows): recorded from the library while the 1x1 launcher existed once per form and all
backward ops were cases of one switch.  The rows of _gnb_new_rows are the exception: the library they would have been
recorded from divides by zero on them.

Not in the table, because a HIP call comes first: a failed hipFuncSetAttribute of the implicit GEMM ("hipFuncSetAttribute:
..." with XL_ERR_HIP) and of the LDS-DMA F(6x6) output transform, the XL_CONV_CLK allocation and copies, the stem launchers'
check of the statistics slots (nchunks, groups), which stands behind XlLdsLimit::configure, and the launch errors xl_cnn_run
collects with hipGetLastError() at the end of a list.  Likewise everything behind XlLdsLimit::configure in the 1x1 and the
persistent launchers (they have no refusal there), the missing pointers of XL_OP_CONV1_WGRAD's fold form on frames wide enough
to need more than 64 KiB of LDS, the hipMemsetAsync of XL_OP_FILL0 and the copies of XL_OP_DUC_HEAD_BWD; XL_OP_GNB_PARAMS and
XL_OP_WINO_WFINAL refuse nothing.  XL_OP_STEM12 and XL_OP_S2_DGRAD have no rows yet."""
import ctypes

import pytest

from crossloc_amd import ops

ARG, UNSUPPORTED = -1, -4
_BUF = ctypes.create_string_buffer(256)
P = ctypes.addressof(_BUF)              # a dummy non-null pointer, and a second one that differs
Q = P + 64
A = (P + 15) & ~15                      # ... and one on a 16-byte boundary, for the launchers that check it (A + 64 is inside _BUF)

WGRAD = ops.XL_OP_WGRAD
CONV1, CONV, GN_STATS, GN_APPLY, HEAD = ops.XL_OP_CONV1, ops.XL_OP_CONV, ops.XL_OP_GN_STATS, ops.XL_OP_GN_APPLY, ops.XL_OP_HEAD
GN_FINAL, WINO_IN, WINO_OUT, DUC_HEAD = ops.XL_OP_GN_FINAL, ops.XL_OP_WINO_IN, ops.XL_OP_WINO_OUT, ops.XL_OP_DUC_HEAD
DGRAD, ACC, SPLIT, IL, PAIR = ops.CONV_DGRAD, ops.CONV_ACCUMULATE, ops.CONV_SPLIT_BF16, ops.CONV_SPLIT_IL, ops.CONV_PAIR_F16
NORM_IN, TILE_MAJOR, GN_ADD = ops.CONV_NORM_IN, ops.CONV_M_TILE_MAJOR, ops.GN_ADD
NORM_RELU, NORM_ADD, ACT, AMAX = ops.CONV_NORM_RELU, ops.CONV_NORM_ADD, ops.CONV_SPLIT_ACT, ops.CONV_PAIR_AMAX
FILL0, GNB_STATS, GNB_FINAL, GNB_APPLY = ops.XL_OP_FILL0, ops.XL_OP_GNB_STATS, ops.XL_OP_GNB_FINAL, ops.XL_OP_GNB_APPLY
GNB_PARAMS_LIST, HEAD_BWD, DUC_HEAD_BWD = ops.XL_OP_GNB_PARAMS_LIST, ops.XL_OP_HEAD_BWD, ops.XL_OP_DUC_HEAD_BWD
WINO_DY, CONV1_WGRAD = ops.XL_OP_WINO_DY, ops.XL_OP_CONV1_WGRAD


def _conv(**kw):
    """a well-formed 3x3 stride-1 64 -> 64 convolution over 16 x 16 pixels, then the fault"""
    d = dict(type=CONV, B=1, Hi=16, Wi=16, Cin=64, Ho=16, Wo=16, Cout=64, ksize=3, stride=1, ld_in=64, ld_out=64)
    d.update(kw)
    return d


def _c1(**kw):
    """the inference form of conv1 (3 -> 32) on a 16 x 64 image: one tile of the matrix-pipe form"""
    d = dict(type=CONV1, B=1, Hi=16, Wi=64, Cin=3, Cout=32, ld_out=32, nchunks=1, groups=32, stats=P)
    d.update(kw)
    return d


def _win(m, **kw):
    d = dict(type=WINO_IN, B=1, Hi=12, Wi=12, Cin=128, Ho=12 // m, Wo=12 // m, ksize=m, ld_in=128, ld_out=128)
    d.update(kw)
    return d


def _wout(m, **kw):
    """12 x 12 output pixels, 4 tiles per workgroup"""
    tiles = (12 // m) ** 2
    d = dict(type=WINO_OUT, B=1, Hi=12, Wi=12, Cin=128, ksize=m, ld_out=128, reserved_i=4, nchunks=(tiles + 3) // 4)
    d.update(kw)
    return d


def _head(**kw):
    d = dict(type=HEAD, B=1, Hi=4, Wi=4, Cin=512, Cout=4, ld_in=512, n_task=3, n_pos=1)
    d.update(kw)
    return d


def _duc(**kw):
    d = dict(type=DUC_HEAD, B=1, Hi=2, Wi=2, Cin=384, Cout=6, Ho=16, Wo=16, ld_in=384)
    d.update(kw)
    return d


def _gn(t, **kw):
    d = dict(type=t, B=1, Hi=16, Wi=16, Cin=64, groups=32, nchunks=4, ld_in=64, ld_out=64)
    d.update(kw)
    return d


def _s2(pair, extra=0, **kw):
    """a well-formed 3x3 stride-2 64 -> 128 stem convolution, 64 x 64 -> 32 x 32 pixels, in the six-pass or the pair form"""
    d = dict(type=CONV, B=1, Hi=64, Wi=64, Cin=64, Ho=32, Wo=32, Cout=128, ksize=3, stride=2, ld_in=64, ld_out=128,
             flags=SPLIT | IL | (PAIR if pair else 0) | extra, w=A, out=A, bias=A, scale=A if pair else 0, **{"in_": A})
    d.update(kw)
    return d


def _s2_rows():
    """every clause of the stem launchers' one refusing statement that xl_run_conv lets through, for both forms"""
    rows = []
    for pair, form in ((False, "s2-split-"), (True, "s2-pair-")):
        rows += [(form + name, _s2(pair, **kw), ARG, None) for name, kw in (
            ("cin", dict(Cin=96, ld_in=96)),
            ("cout", dict(Cout=96, ld_out=96)),
            ("rows", dict(Ho=31)),
            ("columns", dict(Wo=31)),
            ("image-below-tile", dict(Hi=30, Wi=30, Ho=15, Wo=15)),
            ("ld-in-below-cin", dict(ld_in=32)),
            ("ld-out-below-cout", dict(ld_out=64)),
            ("ld-out-4", dict(ld_out=130)),
            ("no-bias", dict(bias=0)),
            ("accumulate", dict(extra=ACC)),
            ("no-input", {"in_": 0}),
            ("no-weights", dict(w=0)),
            ("no-output", dict(out=0)),
            ("stats-alignment", dict(stats=A + 8, groups=32, nchunks=64)),
            ("input-alignment", {"in_": A + 4}),
            ("weight-alignment", dict(w=A + 8)),
            ("output-alignment", dict(out=A + 4)),
            ("pixels-2gib", dict(B=1 << 21)),
            ("two-images-2gib", dict(Hi=4096, Wi=4096, Ho=2048, Wo=2048)),
            ("tile-rows-2gib", dict(ld_out=1 << 21)),
            ("norm-no-coefficients", dict(extra=NORM_IN)),
        )]
    rows.append(("s2-pair-no-scale", _s2(True, scale=0), ARG, None))
    # the pair flag alone chooses the pair launcher (xl_run_conv asks for it first), which then misses the scale
    rows.append(("s2-pair-flag-before-split-flag", _s2(True, flags=PAIR, scale=0), ARG, None))
    return rows


def _wg(pair, splits, extra=0, **kw):
    """a well-formed 64 -> 64 weight-gradient product over 16 x 16 pixels on the split (pair) pipe; with one split the result
    goes to `out`, with more the partial tiles to `stats2`"""
    d = dict(type=WGRAD, B=1, Hi=16, Wi=16, Cin=64, Ho=16, Wo=16, Cout=64, ksize=1, stride=1, ld_in=64, ld_aux=64,
             nchunks2=splits, flags=SPLIT | (PAIR if pair else 0) | extra, aux=A, out=A, stats2=A,
             scale=A if pair else 0, out2=A if pair else 0, **{"in_": A})
    d.update(kw)
    return d


def _wg_rows():
    """every refusing statement of the weight-gradient launchers behind the checks of xl_run_wgrad, for both forms, with one
    split (the launcher gets `out` as its partial tile) and with four"""
    rows = []
    for pair, form in ((False, "wgrad-split-"), (True, "wgrad-pair-")):
        for splits in (1, 4):
            tag = form + "%d-" % splits
            rows += [(tag + name, _wg(pair, splits, **kw), ARG, None) for name, kw in (
                ("ksize", dict(ksize=3)),
                ("stride", dict(stride=2)),
                ("cin-4", dict(Cin=66, ld_in=68)),
                ("no-input", {"in_": 0}),
                ("no-dy", dict(aux=0)),
                ("no-partial", dict(out=0) if splits == 1 else dict(stats2=0)),
                ("norm-no-coefficients", dict(extra=NORM_IN)),
                ("norm-batched", dict(extra=NORM_IN, aux2=A, groups=4)),
                ("norm-pixels-8", dict(extra=NORM_IN, aux2=A, Hi=15, Wi=15, Ho=15, Wo=15)),
                ("batched-ld-in", dict(groups=4, ld_in=68)),
                ("batched-ld-aux", dict(groups=4, ld_aux=68)),
                ("x-2gib", dict(Hi=4096, Wi=4096, Ho=4096, Wo=4096, Cout=4, ld_aux=4)),
                ("dy-2gib", dict(Hi=4096, Wi=4096, Ho=4096, Wo=4096, Cin=4, ld_in=4)),
            )]
            if pair:
                rows += [(tag + "no-scale", _wg(True, splits, scale=0), ARG, None),
                         (tag + "no-amax", _wg(True, splits, out2=0), ARG, None)]
    # with the split flag the launcher's own check answers; without it the same shape has no fp32 kernel
    rows.append(("wgrad-split-ksize-before-fp32-shapes", _wg(False, 4, ksize=3, Cin=48, ld_in=48, Cout=48, ld_aux=48), ARG, None))
    rows.append(("wgrad-fp32-shapes", _wg(False, 4, flags=0, Cin=48, ld_in=48, Cout=48, ld_aux=48), UNSUPPORTED, None))
    return rows


def _g1(pair, extra=0, **kw):
    """a well-formed 1x1 32 -> 256 convolution over 16 x 16 pixels (one 256-row tile) on the split (pair) pipe"""
    d = dict(type=CONV, B=1, Hi=16, Wi=16, Cin=32, Ho=16, Wo=16, Cout=256, ksize=1, stride=1, ld_in=32, ld_out=256,
             flags=SPLIT | IL | (PAIR if pair else 0) | extra, w=A, out=A, scale=A if pair else 0, **{"in_": A})
    d.update(kw)
    return d


def _g1_rows():
    """every clause of the refusing statements of the 1x1 / XL_CONV_SPLIT_ACT launcher (csrc/xl_conv1x1.h) that xl_run_conv lets
    through, for both operand forms.  `half` (`quarter`) is an image below one 256-row (128-row) tile; Z = 4 stands for the
    batched products of a Winograd layer.  Two clauses have no row because an earlier statement answers the same op with the
    same status: the Z > 1 of XL_CONV_NORM_ADD (it needs XL_CONV_NORM_IN, which the first statement refuses for Z > 1) and the
    ld_out of XL_CONV_M_TILE_MAJOR (the first statement's, for Z > 1)."""
    half = dict(Hi=8, Wi=16, Ho=8, Wo=16)
    quarter = dict(Hi=8, Wi=8, Ho=8, Wo=8)
    z4 = dict(nchunks2=4, extra=ACT)
    add = dict(extra=NORM_IN | NORM_RELU | NORM_ADD, aux2=A, aux=A, ld_aux=32)
    rows = []
    for pair, form in ((False, "1x1-split-"), (True, "1x1-pair-")):
        wide = 524288 if pair else 349536                          # 1024 x Cin weights of 4 (6) bytes reach 2^31 bytes
        rows += [(form + name, _g1(pair, **kw), ARG, None) for name, kw in (
            ("ksize", dict(ksize=5)),
            ("stride", dict(stride=2)),
            ("cin-32", dict(Cin=48, ld_in=48)),
            ("cout-256", dict(Cout=128, ld_out=128)),
            ("cout-max", dict(Cout=1280, ld_out=1280)),
            ("ld-in-below-cin", dict(Cin=64)),
            ("ld-out-below-cout", dict(ld_out=128)),
            ("ld-in-4", dict(ld_in=34)),
            ("ld-out-4", dict(ld_out=258)),
            ("accumulate-norm", dict(extra=ACC | NORM_IN, aux2=A)),
            ("accumulate-batched", dict(nchunks2=4, extra=ACT | ACC)),
            ("accumulate-stats", dict(extra=ACC, stats=A, groups=16, nchunks=2)),
            ("no-input", {"in_": 0}),
            ("no-weights", dict(w=0)),
            ("no-output", dict(out=0)),
            ("input-alignment", {"in_": A + 4}),
            ("weight-alignment", dict(w=A + 8)),
            ("output-alignment", dict(out=A + 4)),
            ("pixels-2gib", dict(B=1 << 23)),
            ("weights-2gib", dict(Cin=wide, ld_in=wide, Cout=1024, ld_out=1024)),
            ("tile-rows-in-2gib", dict(ld_in=1 << 21)),
            ("tile-rows-out-2gib", dict(ld_out=1 << 21)),
            ("batched-bias", dict(bias=A, **z4)),
            ("batched-stats", dict(stats=A, groups=16, nchunks=2, **z4)),
            ("batched-norm", dict(nchunks2=4, extra=ACT | NORM_IN, aux2=A)),
            ("batched-per-image-tiles", dict(reserved_i=-256, **z4)),
            ("batched-ld-in", dict(ld_in=64, **z4)),
            ("batched-ld-out", dict(ld_out=512, **z4)),
            ("norm-no-coefficients", dict(extra=NORM_IN)),
            ("norm-cin-max", dict(extra=NORM_IN, aux2=A, Cin=544, ld_in=544)),
            ("norm-image-below-256", dict(extra=NORM_IN, aux2=A, **half)),
            ("norm-image-below-128", dict(extra=NORM_IN, aux2=A, reserved_i=128, **quarter)),
            ("stats-no-groups", dict(stats=A, groups=0, nchunks=2)),
            ("stats-16-per-group", dict(stats=A, groups=8, nchunks=2)),
            ("stats-image-below-256", dict(stats=A, groups=16, nchunks=2, **half)),
            ("stats-image-below-128", dict(stats=A, groups=16, nchunks=2, reserved_i=128, **quarter)),
            ("stats-slots-256", dict(stats=A, groups=16, nchunks=1)),
            ("stats-slots-128", dict(stats=A, groups=16, nchunks=2, reserved_i=128)),
            ("per-image-below-256", dict(reserved_i=-256, **half)),
            ("per-image-below-128", dict(reserved_i=-128, **quarter)),
            ("add-no-norm", dict(add, extra=NORM_RELU | NORM_ADD)),
            ("add-no-relu", dict(add, extra=NORM_IN | NORM_ADD)),
            ("add-no-residual", dict(add, aux=0)),
            ("add-ld-below-cin", dict(add, Cin=64, ld_in=64)),
            ("add-ld-4", dict(add, ld_aux=34)),
            ("add-alignment", dict(add, aux=A + 4)),
            ("add-tile-rows-2gib", dict(add, ld_aux=1 << 21)),
            ("tile-major-one-product", dict(extra=TILE_MAJOR)),
            ("tile-major-tile-rows-2gib", dict(nchunks2=2048, extra=ACT | TILE_MAJOR, Cout=1024, ld_out=1024)),
        )]
    rows.append(("1x1-pair-no-scale", _g1(True, scale=0), ARG, None))
    rows.append(("pair-not-interleaved", _g1(True, flags=SPLIT | PAIR), ARG, None))
    return rows


def _gb(form, extra=0, **kw):
    """four well-formed batched 32 -> 256 products over 256 rows for a persistent launcher: the split pipe's first form
    ("planes"), its interleaved form ("il") and the pair pipe's ("pair")"""
    d = dict(type=CONV, B=1, Hi=16, Wi=16, Cin=32, Ho=16, Wo=16, Cout=256, ksize=1, stride=1, ld_in=32, ld_out=256, nchunks2=4,
             flags=SPLIT | {"planes": 0, "il": IL, "pair": IL | PAIR}[form] | extra, w=A, out=A, scale=A if form == "pair" else 0,
             **{"in_": A})
    d.update(kw)
    return d


def _gb_rows():
    """every clause of the refusing statements of xl_run_split_gemm (both forms) and xl_run_pair_gemm that xl_run_conv lets
    through; the 32-bit bounds are reached with many images or channels, each shape chosen so that the clauses in front of the
    named one hold.  (Z < 1 reaches only the first form: the interleaved ones go to the 1x1 launcher with nchunks2 <= 1.)"""
    one = dict(Hi=1, Wi=1, Ho=1, Wo=1)
    rows = []
    for form in ("planes", "il", "pair"):
        tag = "batched-%s-" % form
        rows += [(tag + name, _gb(form, **kw), ARG, None) for name, kw in (
            ("ksize", dict(ksize=5)),
            ("stride", dict(stride=2)),
            ("ld-in", dict(ld_in=64)),
            ("ld-out", dict(ld_out=512)),
            ("bias", dict(bias=A)),
            ("stats", dict(stats=A)),
            ("accumulate", dict(extra=ACC)),
            ("no-input", {"in_": 0}),
            ("no-weights", dict(w=0)),
            ("no-output", dict(out=0)),
        )]
        if form != "planes":
            k = 4 if form == "pair" else 6                            # operand bytes per element
            acts, wts = 2048 // k // 32 * 32 + 32, (1 << 23) // k // 32 * 32 + 32      # 2^20 rows (256 rows) of them reach 2^31 bytes
            rows += [(tag + name, _gb(form, **kw), ARG, None) for name, kw in (
                ("cout-256", dict(Cout=128, ld_out=128)),
                ("result-rows-4gib", dict(Cout=1 << 22, ld_out=1 << 22, **one)),
                ("activations-2gib", dict(B=4096, Cin=acts, ld_in=acts)),
                ("weights-2gib", dict(Cin=wts, ld_in=wts, **one)),
                ("result-2gib", dict(B=8192)),
            )]
    rows += [("batched-planes-" + name, _gb("planes", **kw), ARG, None) for name, kw in (
        ("no-products", dict(nchunks2=0)),
        ("cin-32", dict(Cin=48, ld_in=48)),
        ("activations-2gib", dict(B=1 << 15)),
        ("weights-2gib", dict(Cin=8192, ld_in=8192, Cout=32768, ld_out=32768)),
        ("result-2gib", dict(B=2048)),
    )]
    rows += [("batched-pair-" + name, _gb("pair", **kw), ARG, None) for name, kw in (
        ("norm", dict(extra=NORM_IN)),
        ("tile-major", dict(extra=TILE_MAJOR)),
        ("amax", dict(extra=AMAX)),
        ("no-scale", dict(scale=0)),
        ("input-alignment", {"in_": A + 4}),
        ("weight-alignment", dict(w=A + 8)),
        ("output-alignment", dict(out=A + 4)),
    )]
    return rows


def _gnb(t, **kw):
    d = dict(type=t, B=1, Hi=16, Wi=16, Cin=64, groups=32, nchunks2=4, ld_in=64, ld_aux=64, ld_out=64, stats=P, stats2=P)
    d.update(kw)
    return d


def _wdy(m, **kw):
    d = dict(type=WINO_DY, B=1, Hi=12, Wi=12, Cin=64, Ho=12 // m, Wo=12 // m, ksize=m, ld_in=64)
    d.update(kw)
    return d


def _c1w(**kw):
    """the weight gradient of conv1 (3 -> 32) on a 16 x 64 image"""
    d = dict(type=CONV1_WGRAD, B=1, Hi=16, Wi=64, Cin=3, Cout=32, ld_aux=32, ld_in=32)
    d.update(kw)
    return d


def _bwd_rows():
    """every refusing statement of the backward launchers that is reached before the first HIP call (the weight-gradient
    products on the matrix pipe are in _wg_rows)"""
    fp32 = dict(flags=0)                                                  # XL_OP_WGRAD on the exact-fp32 kernel, 64 -> 64
    rows = [
        ("fill0-no-output", dict(type=FILL0, Cin=8), ARG, None),
        ("fill0-no-bytes", dict(type=FILL0, out=P), ARG, None),
        ("wgrad-no-splits", _wg(False, 0, **fp32), ARG, None),
        ("wgrad-ld-in-4", _wg(False, 4, ld_in=66, **fp32), ARG, None),
        ("wgrad-ld-aux-4", _wg(False, 4, ld_aux=66, **fp32), ARG, None),
        ("wgrad-no-splits-before-fp32-shapes", _wg(False, 0, Cin=48, ld_in=48, Cout=48, ld_aux=48, **fp32), ARG, None),
        ("wgrad-fp32-batched-ksize", _wg(False, 4, groups=4, ksize=3, **fp32), ARG, None),
        ("wgrad-fp32-batched-ld-in", _wg(False, 4, groups=4, ld_in=68, **fp32), ARG, None),
        ("wgrad-fp32-batched-ld-aux", _wg(False, 4, groups=4, ld_aux=68, **fp32), ARG, None),
        ("wgrad-fp32-x-2gib", _wg(False, 4, Hi=4096, Wi=4096, **fp32), ARG, None),
        ("wgrad-fp32-dy-2gib", _wg(False, 4, Ho=4096, Wo=4096, **fp32), ARG, None),
        ("wgrad-fp32-image-below-k-step", _wg(False, 4, Hi=4, Wi=4, Ho=4, Wo=4, **fp32), UNSUPPORTED, None),
        ("wgrad-fp32-x-2gib-before-image", _wg(False, 4, Hi=4096, Wi=4096, Ho=4, Wo=4, **fp32), ARG, None),
    ]
    for t, tag in ((GNB_STATS, "gnb-stats-"), (GNB_FINAL, "gnb-final-"), (GNB_APPLY, "gnb-apply-")):
        rows += [(tag + name, _gnb(t, **kw), ARG, None) for name, kw in (
            ("cin-4", dict(Cin=66, groups=33)),
            ("groups-divide", dict(groups=24)),
            ("groups-max", dict(Cin=128, groups=128)),
            ("no-chunks", dict(nchunks2=0)),
            ("no-forward-table", dict(stats=0)),
            ("no-scratch", dict(stats2=0)),
        )]
    rows += [
        # 17 channel quads: the first multiple of 17 threads that is whole waves is 17 * 64 = 1088 > 1024
        ("gnb-stats-no-thread-count", _gnb(GNB_STATS, Cin=68, groups=4), ARG, None),
        ("gnb-stats-threads-max", _gnb(GNB_STATS, Cin=4112, groups=16), ARG, None),
        ("gnb-params-list-no-layers", dict(type=GNB_PARAMS_LIST, Cin=0, Cout=64, **{"in_": P}), ARG, None),
        ("gnb-params-list-layers-max", dict(type=GNB_PARAMS_LIST, Cin=65536, Cout=64, **{"in_": P}), ARG, None),
        ("gnb-params-list-no-items", dict(type=GNB_PARAMS_LIST, Cin=4, Cout=64), ARG, None),
        ("gnb-params-list-no-channels", dict(type=GNB_PARAMS_LIST, Cin=4, Cout=0, **{"in_": P}), ARG, None),
        ("head-bwd-cin-4", _head(type=HEAD_BWD, Cin=6, ld_in=8), ARG, None),
        ("head-bwd-cin-min", _head(type=HEAD_BWD, Cin=0), ARG, None),
        ("head-bwd-cin-max", _head(type=HEAD_BWD, Cin=1028, ld_in=1028), ARG, None),
        ("head-bwd-cout-max", _head(type=HEAD_BWD, Cout=5), ARG, None),
        ("head-bwd-cout-min", _head(type=HEAD_BWD, Cout=0), ARG, None),
        ("duc-head-bwd-cout-min", _duc(type=DUC_HEAD_BWD, Cout=0, Cin=0), ARG, None),
        ("duc-head-bwd-cout-max", _duc(type=DUC_HEAD_BWD, Cout=9, Cin=576), ARG, None),
        ("duc-head-bwd-cin", _duc(type=DUC_HEAD_BWD, Cin=320), ARG, None),
    ]
    for m in (4, 6):
        rows += [("wino%d-dy-%s" % (m, name), _wdy(m, **kw), ARG, None) for name, kw in (
            ("cin-2", dict(Cin=63)),
            ("ld-2", dict(ld_in=65)),
            ("tile-rows", dict(Hi=13)),
            ("tile-columns", dict(Wi=13)),
        )]
    rows += [
        ("conv1-wgrad-cout", _c1w(Cout=64), UNSUPPORTED, None),
        ("conv1-wgrad-cin", _c1w(Cin=4), UNSUPPORTED, None),
        ("conv1-wgrad-ld-aux-4", _c1w(ld_aux=34), ARG, None),
        ("conv1-wgrad-cout-before-ld-aux", _c1w(Cout=64, ld_aux=34), UNSUPPORTED, None),
        ("conv1-wgrad-width", _c1w(Wi=2559), UNSUPPORTED, None),
        ("conv1-wgrad-ld-aux-before-width", _c1w(Wi=2559, ld_aux=34), ARG, None),
        ("conv1-wgrad-fold-no-table", _c1w(aux2=P, bias=P), ARG, None),
        ("conv1-wgrad-fold-no-coefficients", _c1w(aux2=P, w=P), ARG, None),
        ("conv1-wgrad-fold-ld-in-4", _c1w(aux2=P, w=P, bias=P, ld_in=34), ARG, None),
    ]
    return rows


def _gnb_new_rows():
    """NOT recorded from the library before the backward launchers were split: there these ops divide by zero (Cin % groups,
    256 % (Cin / 4), 64 % (Cin / groups)) and kill the process.  xl_run_gnb refuses them before it divides."""
    rows = []
    for t, tag in ((GNB_STATS, "gnb-stats-"), (GNB_FINAL, "gnb-final-"), (GNB_APPLY, "gnb-apply-")):
        rows += [(tag + "no-groups", _gnb(t, groups=0), ARG, None), (tag + "no-channels", _gnb(t, Cin=0), ARG, None)]
    rows.append(("gnb-stats-negative-groups", _gnb(GNB_STATS, groups=-4), ARG, None))
    return rows


# (name, op fields, status, piece of the error text or None)
TABLE = [
    # ---- XL_OP_CONV1: matrix-pipe inference form, VALU inference form, direct form
    ("conv1-mfma-tile-count", _c1(nchunks=2), ARG, None),
    ("conv1-mfma-groups", _c1(groups=16), ARG, None),
    ("conv1-fused-cin", _c1(Cin=4, reserved_i=1), ARG, None),
    ("conv1-fused-cout", _c1(Cout=64, reserved_i=4), ARG, None),
    ("conv1-fused-ld", _c1(ld_out=64, reserved_i=4), ARG, None),
    ("conv1-fused-negative-form", _c1(reserved_i=-1), ARG, None),
    ("conv1-fused-too-few-chunks", _c1(reserved_i=1, nchunks=3), ARG, None),
    ("conv1-fused-groups", _c1(reserved_i=4, groups=16), ARG, None),
    ("conv1-fused-apply-cout", _c1(stats=0, aux2=P, Cout=16, reserved_i=4), ARG, None),
    ("conv1-direct-cout-8", dict(type=CONV1, B=1, Hi=8, Wi=8, Cin=3, Cout=12, ld_out=12), ARG, None),
    ("conv1-direct-cout-max", dict(type=CONV1, B=1, Hi=8, Wi=8, Cin=3, Cout=72, ld_out=72), ARG, None),
    ("conv1-direct-threads-per-pixel", dict(type=CONV1, B=1, Hi=8, Wi=8, Cin=3, Cout=24, ld_out=24), ARG, None),
    ("conv1-direct-ld", dict(type=CONV1, B=1, Hi=8, Wi=8, Cin=3, Cout=32, ld_out=34), ARG, None),
    # ---- XL_OP_CONV: dispatch
    ("conv-cin-32", _conv(Cin=48), ARG, None),
    ("conv-cout-32", _conv(Cout=48), ARG, None),
    ("conv-ld-in", _conv(ld_in=66), ARG, None),
    ("conv-cin-before-ksize", _conv(Cin=48, ksize=5), ARG, None),
    ("conv-ksize", _conv(ksize=5), UNSUPPORTED, None),
    ("conv-ksize-before-ld-out", _conv(ksize=5, ld_out=66), UNSUPPORTED, None),
    ("conv-1x1-stride-2", _conv(ksize=1, stride=2), UNSUPPORTED, None),
    ("conv-3x3-stride-3", _conv(stride=3), UNSUPPORTED, None),
    ("conv-dgrad-ksize", _conv(flags=DGRAD, ksize=5), UNSUPPORTED, None),
    ("conv-dgrad-stride", _conv(flags=DGRAD, stride=3), UNSUPPORTED, None),
    ("conv-dgrad-1x1-stride-2", _conv(flags=DGRAD, ksize=1, stride=2), UNSUPPORTED, None),
    ("conv-wino-batch-narrow", _conv(ksize=1, nchunks2=16), UNSUPPORTED, None),
    ("conv-wino-batch-narrow-before-stats", _conv(ksize=1, nchunks2=16, stats=P, groups=32), UNSUPPORTED, None),
    ("conv-norm-narrow", _conv(ksize=1, flags=NORM_IN, aux2=P), UNSUPPORTED, None),
    ("conv-norm-small-tiles", _conv(ksize=1, Cout=128, ld_out=128, flags=NORM_IN, aux2=P, reserved_i=64), UNSUPPORTED, None),
    ("conv-norm-small-tiles-before-coefficients", _conv(ksize=1, Cout=128, ld_out=128, flags=NORM_IN, reserved_i=64), UNSUPPORTED, None),
    # ---- XL_OP_CONV: the launcher
    ("conv-norm-no-coefficients", _conv(ksize=1, Cout=128, ld_out=128, flags=NORM_IN), ARG, None),
    ("conv-norm-image-below-tile", _conv(ksize=1, Cout=128, ld_out=128, flags=NORM_IN, aux2=P, Hi=8, Wi=8, Ho=8, Wo=8), ARG, None),
    ("conv-wino-batch-stats", _conv(ksize=1, Cout=128, ld_out=128, nchunks2=16, stats=P, groups=32), ARG, None),
    ("conv-wino-batch-stats-before-ld-out", _conv(ksize=1, Cout=128, ld_out=130, nchunks2=16, stats=P, groups=32), ARG, None),
    ("conv-stats-image-below-tile", _conv(stats=P, groups=32, nchunks=8, Hi=8, Wi=8, Ho=8, Wo=8), ARG, None),
    ("conv-stats-groups-divide", _conv(stats=P, groups=24, nchunks=8), ARG, None),
    ("conv-stats-group-in-tile", _conv(Cout=96, ld_out=96, stats=P, groups=2, nchunks=8), ARG, None),
    ("conv-stats-too-few-slots", _conv(stats=P, groups=32, nchunks=2), ARG, None),
    ("conv-stats-piece", _conv(stats=P, groups=64, nchunks=8), ARG, None),
    ("conv-weight-bytes", _conv(Cin=8192, Cout=8192, ld_in=8192, ld_out=8192), ARG, "conv weights of 2415919104 bytes"),
    ("conv-weight-bytes-before-ld-out", _conv(Cin=8192, Cout=8192, ld_in=8192, ld_out=8194), ARG, "conv weights of"),
    ("conv-2gib-one-image", _conv(Hi=4096, Wi=4096, Ho=4096, Wo=4096, Cin=32, ld_in=32), ARG, "exceed 32-bit buffer addressing"),
    ("conv-2gib-dgrad-s2", _conv(flags=DGRAD, stride=2, B=64, Hi=512, Wi=512, Ho=1024, Wo=1024), ARG, "exceed 32-bit buffer addressing"),
    ("conv-2gib-wino-batch", _conv(ksize=1, Cin=128, ld_in=128, Cout=128, ld_out=128, nchunks2=16, B=64, Hi=256, Wi=256, Ho=256, Wo=256),
     ARG, "exceed 32-bit buffer addressing"),
    ("conv-ld-out", _conv(ld_out=66), ARG, None),
    ("conv-dgrad-bias", _conv(flags=DGRAD, bias=P), ARG, None),
    ("conv-wino-batch-bias", _conv(ksize=1, Cout=128, ld_out=128, nchunks2=16, bias=P), ARG, None),
    ("conv-accumulate-stats", _conv(flags=ACC, stats=P, groups=32, nchunks=8), ARG, None),
    # ---- XL_OP_WINO_IN
    ("wino6-in-cin", _win(6, Cin=126, ld_in=126), ARG, None),
    ("wino6-in-ld", _win(6, ld_in=129), ARG, None),
    ("wino6-in-tile-rows", _win(6, Hi=13), ARG, None),
    ("wino6-in-tile-columns", _win(6, Wi=13), ARG, None),
    ("wino6-in-interleaved-cin", _win(6, Cin=192, ld_in=192, flags=SPLIT | IL), ARG, None),
    ("wino6-in-fold-no-coefficients", _win(6, out2=P), ARG, None),
    ("wino6-in-fold-ld-side", _win(6, out2=P, aux2=Q, ld_out=129), ARG, None),
    ("wino6-in-fold-no-residual", _win(6, out2=P, aux2=Q, flags=GN_ADD), ARG, None),
    ("wino6-in-fold-ld-residual", _win(6, out2=P, aux2=Q, flags=GN_ADD, aux=Q, ld_aux=129), ARG, None),
    ("wino6-in-fold-aliases-input", _win(6, out2=P, aux2=Q, **{"in_": P}), ARG, None),
    ("wino6-in-fold-aliases-residual", _win(6, out2=P, aux2=Q, flags=GN_ADD, aux=P, ld_aux=128), ARG, None),
    ("wino6-in-fold-bf16", _win(6, out2=P, aux2=Q, flags=SPLIT), UNSUPPORTED, None),
    ("wino6-in-pair-no-scale", _win(6, flags=PAIR), ARG, None),
    ("wino6-in-pair-cin", _win(6, Cin=72, ld_in=72, flags=PAIR, scale=P), ARG, None),
    ("wino4-in-cin", _win(4, Cin=126, ld_in=126), ARG, None),
    ("wino4-in-ld", _win(4, ld_in=129), ARG, None),
    ("wino4-in-tile-rows", _win(4, Hi=13), ARG, None),
    ("wino4-in-tile-columns", _win(4, Wi=13), ARG, None),
    ("wino2-in-deferred-norm", _win(2, aux2=P), ARG, None),
    ("wino2-in-cin", _win(2, Cin=126, ld_in=128), ARG, None),
    ("wino2-in-ld", _win(2, ld_in=130), ARG, None),
    ("wino2-in-rows", _win(2, Hi=13), ARG, None),
    ("wino2-in-columns", _win(2, Wi=13), ARG, None),
    # ---- XL_OP_WINO_OUT
    ("wino6-out-cin-odd", _wout(6, Cin=127), ARG, None),
    ("wino6-out-cin-block", _wout(6, Cin=384, ld_out=384), ARG, None),
    ("wino6-out-threads", _wout(6, Cin=96, ld_out=96), ARG, None),
    ("wino6-out-ld", _wout(6, ld_out=129), ARG, None),
    ("wino6-out-tiles-per-block", _wout(6, reserved_i=0), ARG, None),
    ("wino6-out-chunks", _wout(6, nchunks=2), ARG, None),
    ("wino6-out-stats-no-groups", _wout(6, stats=P), ARG, None),
    ("wino6-out-stats-groups-divide", _wout(6, stats=P, groups=24), ARG, None),
    ("wino6-out-stats-group-in-block", _wout(6, Cin=768, ld_out=768, stats=P, groups=2), ARG, None),
    ("wino4-out-tile-major", _wout(4, flags=TILE_MAJOR), UNSUPPORTED, None),
    ("wino4-out-tile-major-before-cin", _wout(4, Cin=127, flags=TILE_MAJOR), UNSUPPORTED, None),
    ("wino4-out-cin-odd", _wout(4, Cin=127), ARG, None),
    ("wino4-out-cin-block", _wout(4, Cin=768, ld_out=768), ARG, None),
    ("wino4-out-threads", _wout(4, Cin=96, ld_out=96), ARG, None),
    ("wino4-out-ld", _wout(4, ld_out=129), ARG, None),
    ("wino4-out-tiles-per-block", _wout(4, reserved_i=0), ARG, None),
    ("wino4-out-chunks", _wout(4, nchunks=2), ARG, None),
    ("wino4-out-stats-no-groups", _wout(4, stats=P), ARG, None),
    ("wino4-out-stats-groups-divide", _wout(4, stats=P, groups=24), ARG, None),
    ("wino4-out-stats-group-in-block", _wout(4, Cin=1536, ld_out=1536, stats=P, groups=2), ARG, None),
    ("wino4-out-stats-writers", _wout(4, Cin=512, ld_out=512, stats=P, groups=512), ARG, None),
    ("wino2-out-cin", _wout(2, Cin=126), ARG, None),
    ("wino2-out-cin-max", _wout(2, Cin=2048, ld_out=2048), ARG, None),
    ("wino2-out-threads", _wout(2, Cin=48, ld_out=48), ARG, None),
    ("wino2-out-ld", _wout(2, ld_out=130), ARG, None),
    ("wino2-out-tiles-per-block", _wout(2, reserved_i=0), ARG, None),
    ("wino2-out-rows", _wout(2, Hi=13), ARG, None),
    ("wino2-out-columns", _wout(2, Wi=13), ARG, None),
    ("wino2-out-chunks", _wout(2, nchunks=8), ARG, None),
    ("wino2-out-stats-no-groups", _wout(2, stats=P), ARG, None),
    ("wino2-out-stats-groups-max", _wout(2, Cin=1024, ld_out=1024, stats=P, groups=512), ARG, None),
    ("wino2-out-stats-groups-divide", _wout(2, stats=P, groups=24), ARG, None),
    # ---- GroupNorm
    ("gn-stats-cin", _gn(GN_STATS, Cin=66, groups=33), ARG, None),
    ("gn-stats-groups-divide", _gn(GN_STATS, groups=24), ARG, None),
    ("gn-stats-ld", _gn(GN_STATS, ld_in=66), ARG, None),
    ("gn-stats-threads-max", _gn(GN_STATS, Cin=4100, ld_in=4100, groups=1), ARG, None),
    ("gn-stats-whole-waves", _gn(GN_STATS, Cin=1040, ld_in=1040, groups=1), ARG, None),
    ("gn-stats-groups-max", _gn(GN_STATS, Cin=1024, ld_in=1024, groups=1024), ARG, None),
    ("gn-apply-cin", _gn(GN_APPLY, Cin=66), ARG, None),
    ("gn-apply-ld-in", _gn(GN_APPLY, ld_in=66), ARG, None),
    ("gn-apply-ld-out", _gn(GN_APPLY, ld_out=66), ARG, None),
    ("gn-final-groups-max", _gn(GN_FINAL, groups=64), ARG, None),
    ("gn-final-groups-divide", _gn(GN_FINAL, groups=24), ARG, None),
    ("gn-final-slots", _gn(GN_FINAL, reserved_i=128, nchunks=2), ARG, None),
    ("gn-final-slots-aligned-tiles", _gn(GN_FINAL, reserved_i=-128, nchunks=1), ARG, None),
    ("gn-final-slots-per-tile", _gn(GN_FINAL, reserved_i=-128, stride=2, nchunks=3), ARG, None),
    # ---- heads
    ("head-cin-4", _head(Cin=6, ld_in=8), ARG, None),
    ("head-cin-min", _head(Cin=0), ARG, None),
    ("head-cin-max", _head(Cin=2052, ld_in=2052), ARG, None),
    ("head-cout-max", _head(Cout=9), ARG, None),
    ("head-cout-min", _head(Cout=0), ARG, None),
    ("head-ld", _head(ld_in=514), ARG, None),
    ("head-norm-cin", _head(Cin=256, ld_in=256, aux2=P), UNSUPPORTED, None),
    ("head-norm-cout", _head(Cout=5, aux2=P), UNSUPPORTED, None),
    ("head-cin-before-norm", _head(Cin=6, ld_in=8, aux2=P), ARG, "op 0 refused (type 4, k0 s0, 6 -> 4 channels, in 4x4 out 0x0, B 1, ld 8/0, flags 0x0, Z 0, form 0)"),
    ("duc-head-cout-min", _duc(Cout=0, Cin=0), ARG, None),
    ("duc-head-cout-max", _duc(Cout=9, Cin=576), ARG, None),
    ("duc-head-cin", _duc(Cin=320), ARG, None),
    ("duc-head-rows", _duc(Ho=0), ARG, None),
    ("duc-head-columns", _duc(Wo=0), ARG, "op 0 refused (type 14"),
    # ---- XL_OP_CONV 3x3 stride 2 on the split / pair pipe, XL_OP_WGRAD on the split / pair pipe (one launcher per family)
    *_s2_rows(),
    *_wg_rows(),
    # ---- XL_OP_CONV 1x1 / XL_CONV_SPLIT_ACT on the split / pair pipe (one launcher), the persistent batched GEMMs of both pipes
    *_g1_rows(),
    *_gb_rows(),
    # ---- the backward ops, one launcher per op type in the file of its kernel family
    *_bwd_rows(),
    *_gnb_new_rows(),
    # ---- and an op type that has no launcher
    ("unknown-op-type", dict(type=99), UNSUPPORTED, "op 0 refused (type 99"),
]


@pytest.fixture(scope="module")
def lib():
    return ops._bind()


def test_the_table_has_one_name_per_row():
    names = [row[0] for row in TABLE]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("name,fields,status,text", TABLE, ids=[row[0] for row in TABLE])
def test_a_malformed_op_is_refused_with_its_status(lib, name, fields, status, text):
    op = ops.XlOp()
    for k, v in fields.items():
        assert hasattr(op, k), k
        setattr(op, k, v)
    rc = lib.xl_cnn_run(ctypes.byref(op), 1, None)
    msg = lib.xl_cnn_last_error().decode()
    assert rc == status, (name, rc, msg)
    assert "op 0 refused (type %d" % fields["type"] in msg, msg
    if text is not None:
        assert text in msg, msg
    if text is None or text.startswith("op 0"):
        assert msg.startswith("op 0 refused"), msg                         # no launcher text in front


def test_a_refusal_stops_the_list_and_names_the_index(lib):
    arr = (ops.XlOp * 2)()
    for op in arr:
        for k, v in _head(Cin=6, ld_in=8).items():
            setattr(op, k, v)
    arr[0].Cin, arr[0].ld_in, arr[0].Cout = 512, 512, 9
    assert lib.xl_cnn_run(arr, 2, None) == ARG
    assert "op 0 refused" in lib.xl_cnn_last_error().decode() and "512 -> 9 channels" in lib.xl_cnn_last_error().decode()
    assert lib.xl_cnn_run(None, 1, None) == ARG
    assert lib.xl_cnn_run(arr, -1, None) == ARG
