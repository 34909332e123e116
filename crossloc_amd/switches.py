"""Every Python-side `XL_*` switch, declared once: name, kind, default, meaning.

Three kinds, each with its own truth convention (kept exactly as the scattered reads had them):

  FLAG        off-switches and opt-ins: ON for ANY non-empty value - `XL_NO_WINOGRAD=0` still means "off-switch set"
  DEFAULT_ON  ON unless the value is "" or "0"
  VALUE       the string itself (None / the default when unset); the reader interprets it

A `_Plan` takes ONE snapshot of the lowering switches when it is built (`plan.sw`, attributes named without the `XL_`
prefix): forward lowering, backward lowering and every later `refresh_weights` answer from it, so a plan cannot be lowered
under two environments.  The LIVE switches are read each time they matter (`live(name)`): tests flip them on a live plan.
The C++ side reads further switches of its own with getenv; they are not listed here.
"""
import os

FLAG, DEFAULT_ON, VALUE = "flag", "default_on", "value"

LOWERING = (
    # ---- matrix-pipe forms
    ("XL_GEMM_SPLIT_BF16", VALUE, "il", 'GEMMs on the bf16 matrix pipe, operands split in three exact bf16 terms: "il" = interleaved planes + '
                                        '256 x 256 persistent kernels, "1" = separate planes + 128 x 128 register-staged kernel (Winograd '
                                        'layers only), "0" / "" = fp32 MFMA everywhere'),
    ("XL_GEMM_PAIR", DEFAULT_ON, "1", "forward GEMMs as three fp16-pair passes instead of six bf16 ones (csrc/xl_gemm_pair.hip)"),
    ("XL_TRAIN_PAIR", DEFAULT_ON, "1", "... in training plans too (their forward operands are GroupNorm outputs as well)"),
    ("XL_TRAIN_PAIR_BWD", DEFAULT_ON, "1", "backward GEMMs as fp16 pairs scaled by a recorded max |gradient|; 0: six-pass bf16"),
    ("XL_TRAIN_PAIR_STEM", DEFAULT_ON, "1", "training plans run the stride-2 stem layers as fp16 pairs; 0: the six-pass kernels"),
    ("XL_NO_PAIR_STEM", FLAG, None, "stem layers never as fp16 pairs"),
    ("XL_PAIR_NO_DMA", FLAG, None, "Winograd pair GEMMs form the pairs inside the GEMM instead of reading a V written as pairs"),
    ("XL_NO_SPLIT_TRAIN", FLAG, None, "training plans on fp32 MFMA throughout (the round-2 training plans)"),
    ("XL_NO_SPLIT_1X1", FLAG, None, "1x1 layers (and their data gradients) off the split pipe"),
    ("XL_NO_SPLIT_WGRAD", FLAG, None, "weight gradients off the split pipe"),
    ("XL_NO_SPLIT_STEM", FLAG, None, "stride-2 stem layers off the split pipe"),
    ("XL_NO_S2_DGRAD", FLAG, None, "the stem's data gradients as four parity-class launches of the fp32 implicit GEMM"),
    ("XL_NO_SMALL_TILES", FLAG, None, "always 256 x 256 tiles, no latency tile forms for small batches"),
    ("XL_TILE_FORM_1X1", VALUE, None, "measurement: force the tile form (256 / 192 / 128 / 384) of the 1x1 layers"),
    ("XL_TILE_FORM_WINO", VALUE, None, "measurement: force the tile form of the batched Winograd GEMMs"),
    # ---- Winograd
    ("XL_WINOGRAD", VALUE, "6", "largest output tile m of F(m x m,3x3): 6, 4, or 2 (inference only)"),
    ("XL_NO_WINOGRAD", FLAG, None, "every 3x3 layer through the direct kernel, forward and backward"),
    ("XL_NO_WINOGRAD_TRAIN", FLAG, None, "training plans without Winograd layers (forward and both gradients)"),
    ("XL_NO_WINOGRAD_WGRAD", FLAG, None, "weight gradients of 3x3 layers through the direct kernel"),
    ("XL_NO_KEEP_V", FLAG, None, "training plans transform the input again for the weight gradient instead of keeping V"),
    ("XL_WINO_V_SPLIT", FLAG, None, "the round-2 form: V written as interleaved bf16 planes by the input transform"),
    ("XL_WINO_M_TILE_MAJOR", FLAG, None, "the product M as [tiles][64][C] (no net gain measured at 47 frames; kept for the A/B)"),
    ("XL_WINO_OUT_TPB16", FLAG, None, "output transform: the halving rule for tiles per workgroup instead of equal-length workgroups"),
    ("XL_WINO_OUT_TPB", VALUE, None, "measurement: force the tiles per workgroup of the forward output transform"),
    # ---- GroupNorm placement
    ("XL_NO_FUSED_STATS", FLAG, None, "separate per-image statistics passes (what batch_invariant networks get)"),
    ("XL_NO_DEFERRED_GN", FLAG, None, "every GroupNorm apply as a pass of its own, none left to the consumer's operand load"),
    ("XL_NO_FOLD_GN", FLAG, None, "an apply with several consumers is never left to the first one's input transform"),
    ("XL_NO_AUX_FOLD", FLAG, None, "res2_conv3's apply is not folded into the addition that consumes it"),
    ("XL_NO_ADD_ON_LOAD", FLAG, None, "no GroupNorm + ReLU + residual + ReLU inside a 1x1 layer's operand load"),
    ("XL_NO_NORM_ON_LOAD", FLAG, None, "1x1 layers never normalise their operand on load"),
    ("XL_NO_TRAIN_DEFER", FLAG, None, "training plans materialise every GroupNorm output"),
    ("XL_GNB_PARAMS_PER_LAYER", FLAG, None, "d gamma / d beta / d bias: one launch per layer instead of one for the whole pass"),
    # ---- stem
    ("XL_NO_CONV1_FUSED", FLAG, None, "inference conv1 as convolution, statistics pass, apply pass"),
    ("XL_CONV1_VALU", FLAG, None, "conv1 on the vector ALUs instead of the matrix pipe"),
    ("XL_CONV1_TWO_PASS", FLAG, None, "conv1 evaluated twice (statistics, then normalised output) instead of applied by conv2 on load"),
    ("XL_NO_CONV1_WGRAD_FOLD", FLAG, None, "conv1's GroupNorm-backward apply as a pass, not inside conv1's weight gradient"),
    ("XL_NO_STEM12", FLAG, None, "conv1 and conv2 as two kernels (csrc/xl_stem_fused.hip off)"),
    ("XL_STEM12_TILE", VALUE, None, '"8": the fused stem kernel runs 8-row tiles (its statistics have that many entries)'),
    ("XL_STEM_FORM", FLAG, None, "a stem tile form is forced on the C++ side: no epilogue statistics"),
    ("XL_NO_STEM_STATS", FLAG, None, "stem layers followed by a statistics pass instead of epilogue statistics"),
    ("XL_TRAIN_STEM_STATS", FLAG, None, "opt-in: epilogue statistics of the stem layers in training plans (no gain; flips ReLUs at kinks)"),
    # ---- other
    ("XL_MLR_LAST_DIRECT", FLAG, None, "the round-3 lowering of an MLR encoder's last block, kept for the A/B"),
    ("XL_WGRAD_SMALL_SPLITS_OLD", FLAG, None, "direct weight gradients: split-K for two resident workgroups per CU whatever the tile"),
)

LIVE = (
    ("XL_CNN_GRAPH", VALUE, None, '"0": never replay a plan as a HIP graph, "1": always (inference); unset: plans of at most 8 frames'),
    ("XL_NO_BATCHED_REPACK", FLAG, None, "refresh_weights re-packs the fp16-pair operands one matrix at a time"),
    ("XL_SOLVER_PRIORITY", DEFAULT_ON, "1", "the pose solver's stream runs at high priority (evaluation.py); 0: equal priorities"),
    ("XL_TRAIN_WORKERS", VALUE, None, "data-loading worker processes of the training driver (training.py)"),
)

_BY_NAME = {row[0]: row for row in LOWERING + LIVE}


def read(name, environ=None):
    """The switch's value under its kind's convention: bool for FLAG / DEFAULT_ON, the string (or default) for VALUE."""
    _, kind, default, _ = _BY_NAME[name]
    v = (os.environ if environ is None else environ).get(name, default)
    return v if kind == VALUE else (bool(v) if kind == FLAG else v not in ("", "0"))


_LIVE = {name: (kind, default) for name, kind, default, _ in LIVE}


def live(name):
    """A LIVE switch as the environment has it now (KeyError for any other name); cheap enough for the per-frame path."""
    kind, default = _LIVE[name]
    v = os.environ.get(name, default)
    return v if kind == VALUE else (bool(v) if kind == FLAG else v not in ("", "0"))


class Snapshot:
    """The lowering switches as they were when a plan was built: `sw.NO_WINOGRAD`, `sw.GEMM_PAIR`, `sw.WINOGRAD`, ..."""

    def __init__(self, environ=None):
        for name, _, _, _ in LOWERING:
            setattr(self, name[3:], read(name, environ))

    @property
    def split_on(self):
        """The interleaved-plane split GEMMs (256 x 256 persistent kernels) are selected."""
        return self.GEMM_SPLIT_BF16 not in ("", "0", "1")

    @property
    def wino_train_on(self):
        """Training plans may run a 3x3 layer's forward, data gradient AND weight gradient as Winograd."""
        return not (self.NO_WINOGRAD or self.NO_WINOGRAD_TRAIN or self.NO_WINOGRAD_WGRAD)
