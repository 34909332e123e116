"""Which kernel form a layer gets: the predicates and cost models that the forward and the backward lowering share
(Winograd tile size, split-pipe and fp16-pair eligibility, tile forms, split-K factors).  They answer from the plan's
shape and its switch snapshot `self.sw` only.  Mixed into `networks._Plan`."""


class _Forms:
    # -- fp16 pair / triple operands (round 5, XL_CONV_PAIR_F16): half the matrix-pipe passes of the split-bf16 GEMMs
    def pair_ok(self):
        """The forward GEMMs of a plan run as three fp16 passes instead of six bf16 ones (csrc/xl_gemm_pair.hip) unless
        XL_GEMM_PAIR=0.  Every convolution this applies to reads GroupNorm outputs (and sums of them): their magnitude is
        bounded by the GroupNorm parameters, which is what makes ONE static power-of-two scale per plan safe for fp16."""
        # (training plans, round 5: the FORWARD GEMMs only - their operands are GroupNorm outputs like an inference plan's; the
        #  gradients the backward GEMMs read have no such bound and stay on the six-pass bf16 kernels.  XL_TRAIN_PAIR=0: off)
        if self.train and not self.sw.TRAIN_PAIR:
            return False
        return self.sw.GEMM_PAIR and self.sw.split_on and self.split_train_ok()

    def wino_pick(self, H, W, chan_max, allowed=(6, 4)):
        """Output tile m of F(m x m, 3x3) for an H x W map: the allowed size (capped by XL_WINOGRAD) with the fewest
        multiplies, (m+2)^2 * ceil(H/m) * ceil(W/m); 0 if none.  The transformed tensors V / M hold (m+2)^2 independent
        GEMM operands of [tiles][channels] each: the batched GEMM launch gives every one of them its own buffer
        descriptor (64-bit base, 32-bit offsets inside), so only ONE operand has to stay below 2 GiB, not the tensor."""
        want = int(self.sw.WINOGRAD)
        cands = [m for m in allowed if m <= want]
        cands.sort(key=lambda m: ((m + 2) ** 2 * -(-H // m) * -(-W // m), -m))
        for m in cands:
            T = self.B * -(-H // m) * -(-W // m)
            if T * chan_max * 4 < 2 ** 31 - 1:
                return m
        return 0

    def wino_wgrad_layer_ok(self, H, W, C, Cout):
        """A stride-1 3x3 layer with this input map may get a Winograd weight gradient: the ONE statement of the condition,
        asked by the forward lowering (wino_wgrad_ok) and by the backward lowering that emits the gradient."""
        return H * W >= 64 and C % 64 == 0 and Cout % 128 == 0 and self.sw.wino_train_on

    def wino_wgrad_ok(self, conv, H, W, C, m):
        """The weight gradient of this F(m x m,3x3) layer will be a Winograd one: it then reads the normalised V and never the
        layer's input tensor.  (When the apply is left to this layer, the backward pass takes the forward's tile size `wm`
        instead of re-deriving one: see `xnorm` in lower_backward.conv.)"""
        return (not conv.weight.requires_grad) or (
            m in (4, 6) and self.wino_wgrad_layer_ok(H, W, C, conv.out_channels) and self.B * -(-H // m) * -(-W // m) >= 64)

    def wino_dgrad_m(self, conv, H, W, C):
        """Data gradient of a stride-1 3x3 layer as F(m x m, 3x3) (C = the layer's input channels = gradient channels):
        the tile size, or 0 for the direct MODE 1 kernel."""
        if (conv.kernel_size[0] != 3 or conv.stride[0] != 1 or C not in (128, 256, 512, 1024)
                or conv.out_channels % 32 != 0 or H * W < 64 or self.sw.NO_WINOGRAD or self.sw.NO_WINOGRAD_TRAIN):
            return 0
        return self.wino_pick(H, W, max(C, conv.out_channels))

    def norm_on_load_ok(self, act, conv):
        """The 1x1 forward conv kernel can apply the producer's GroupNorm(+ReLU) to its A operand while loading it (no
        separate apply pass): 128-row x 128-column tiles, whole 32-channel K-steps, at most two images per tile."""
        t, H, W, C, ld, off = act
        cout = conv.out_channels
        # (the tile-count term - small launches run the 64-row form, which has no operand normalisation - depends on the
        #  batch: batch-invariant plans make the choice from the layer alone, see split_1x1_ok; and every apply site, fused
        #  or not, computes fmaf(x, scale, shift), so the two forms agree to the bit anyway)
        fills = self.separate_stats or -(-self.B * H * W // 128) * (cout // 128) > 256
        return (conv.kernel_size[0] == 1 and conv.stride[0] == 1 and cout % 128 == 0 and C % 32 == 0 and H * W >= 128
                and fills and not self.train and not self.sw.NO_NORM_ON_LOAD)

    def split_1x1_ok(self, act, conv):
        """1x1 stride-1 layers of inference plans on the bf16 matrix pipe (csrc/xl_gemm_split.hip, split_conv1x1_kernel):
        weights split once on the host, activations split by the kernel on their way into LDS - fp32-accurate like the
        Winograd GEMMs.  The choice depends on the layer only, never on the batch: a frame's result must not change with
        the batch it is in (a single frame is 44 tiles of 256 x 256: one short round on 44 CUs, about the time the fp32
        kernel needs for its 340 small tiles)."""
        t, H, W, C, ld, off = act
        cout = conv.out_channels
        return (conv.kernel_size[0] == 1 and conv.stride[0] == 1 and self.split_train_ok() and C % 32 == 0 and cout % 256 == 0
                and cout <= 1024 and H * W >= 256 and ld % 4 == 0 and off % 4 == 0
                and self.sw.split_on and not self.sw.NO_SPLIT_1X1)

    def wgrad_split_ok(self, C, Cout):
        """Weight gradients of 1x1 layers and of the batched Winograd products on the split pipe (256 x 256 tiles)."""
        return C % 256 == 0 and Cout % 256 == 0 and self.split_train_ok() and self.sw.split_on and not self.sw.NO_SPLIT_WGRAD

    @staticmethod
    def wgrad_splits(tiles, K):
        """Split-K factor of the split-pipe weight gradient: fill the 256 CUs once, at least 256 rows of K per split."""
        return max(1, min(256 // max(tiles, 1), K // 256))

    @staticmethod
    def split_k(tiles, rows, bo, bc, resident, max_splits):
        """Split-K factor of a weight gradient on the fp32 pipe (`tiles` output tiles of bo x bc, K = `rows` pixels) from a cost
        model in units of one K-step (32 pixels) of a workgroup: rounds of the `resident` workgroups x (K-steps per split + ~8
        steps of prologue / partial-tile store) + the fixed-order reduce pass over the partial tiles (~4 TB/s, one K-step
        ~ 1.8 us).  E.g. 3x3 512->512 at batch 16: 144 tiles x 7 = 1008 workgroups = 1.97 rounds of 386 steps."""
        steps_total = -(-rows // 32)
        best, splits = None, 1
        for cand in range(1, max_splits + 1):
            if cand > max(1, rows // 256):
                break
            rounds = -(-(tiles * cand) // resident)
            cost = rounds * (-(-steps_total // cand) + 8) + (cand + 1) * tiles * bo * bc * 4 / 4e12 / 1.8e-6
            if best is None or cost < best - 1e-9:
                best, splits = cost, cand
        return splits

    def wino_out_tpb(self, m, tiles, cout):
        """Tiles per workgroup of the Winograd output transform of a map of `tiles` tiles per image and `cout` channels."""
        tpb = 32 if m == 2 else 16
        zblocks = max(1, cout // (256 if m == 6 else 512))          # channel blocks of the output-transform grid
        while tpb > 1 and self.B * -(-tiles // tpb) * zblocks < 1024:
            tpb //= 2                                # small batches: more, shorter workgroups (latency-bound otherwise)
        if m == 6 and cout % 512 == 0 and not self.sw.WINO_OUT_TPB16:
            # the two-channels-per-lane form: 2 workgroups of 4 waves are resident per CU (230 VGPRs), so a launch costs
            # (rounds of 512 workgroups) x (tiles per workgroup + a workgroup's start-up, ~half a tile).  47 frames of 150
            # tiles: 15 tiles per workgroup = 470 workgroups of equal length in ONE round (16: nine chunks of 16 and one of 6
            # per image - the round takes 16 tile-times for 13.8 tiles of work per slot)
            zb = cout // 512
            tpb = min(range(1, 17), key=lambda t: (-(-(self.B * -(-tiles // t) * zb) // 512) * (t + 0.5), -t))
        return tpb

    def split_tile_form(self, M, N, Z=1, HW=1 << 30):
        """Tile form of a 1x1 layer / of the Z batched GEMMs of a Winograd layer on the split pipe, as the op's reserved_i:
        256 = 256 x 256 tiles (8 waves), 192 = 256 rows x 128 columns (8 waves), 128 = 128 x 128 (4 waves), 384 = 256 x 256
        for the full rounds + 256 x 128 for the last partial round (two launches over disjoint tile ranges).  The persistent
        kernels run one workgroup per CU, so a launch costs (rounds of 256 tiles) x (time of a tile); the tile times per
        K-step were measured at 60 x 90 (2.05 / 1.30 / 1.10 us).  At 47 frames the large tiles win everywhere; a single frame
        has 44 large tiles for a 1x1 layer (172 small ones: one round at half the tile time) and 128 for a Winograd layer
        (256 of the 256 x 128 form).  Every output element accumulates in the same order in all forms - the convolution
        results are bitwise the same - but the GroupNorm partial sums are per tile: batch-invariant plans keep 256."""
        if self.separate_stats or self.train or self.sw.NO_SMALL_TILES:
            return 256
        forced = self.sw.TILE_FORM_WINO if Z > 1 else self.sw.TILE_FORM_1X1      # measurement switch
        if forced:
            return int(forced) if (HW >= 128 or forced != "128") else 256
        big = -(-M // 256) * (N // 256) * Z
        cands = [(256, -(-big // 256) * 2.05), (192, -(-2 * big // 256) * 1.30)]
        if big > 256 and 0 < 2 * (big % 256) <= 256:     # 384: full rounds of large tiles, the rest as ONE round of 256 x 128
            cands.append((384, big // 256 * 2.05 + 1.30 + 0.15))          # (+ the second launch's pipeline fill)
        if HW >= 128:
            cands.append((128, -(-(-(-M // 128) * (N // 128) * Z) // 256) * 1.10))
        return min(cands, key=lambda c: (c[1], -c[0]))[0]

    def split_train_ok(self):
        """Training plans run their forward GEMMs (and the Winograd data gradients) on the split pipe too (round 3);
        XL_NO_SPLIT_TRAIN=1: fp32 MFMA throughout, the round-2 training plans."""
        return not self.train or not self.sw.NO_SPLIT_TRAIN

    def stem_split_ok(self, act, conv):
        """The stride-2 3x3 stem layers of inference plans on the bf16 matrix pipe (csrc/xl_stem_split.hip): a choice by
        layer, never by batch."""
        t, H, W, C, ld, off = act
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return (conv.kernel_size[0] == 3 and conv.stride[0] == 2 and self.split_train_ok() and C in (32, 64, 128)
                and conv.out_channels in (64, 128, 256) and Ho * Wo >= 256 and ld % 4 == 0 and off % 4 == 0
                and 2 * H * W * ld * 4 < 2 ** 31 - 1
                and self.sw.split_on and not self.sw.NO_SPLIT_STEM)

    def wino_tile(self, act, conv):
        """Stride-1 3x3 convolutions run as Winograd F(m x m, 3x3).  Returns the output tile size m, or 0 for the direct
        kernel.  Inference plans choose between F(6x6,3x3) (64 multiplies per 36 outputs) and F(4x4,3x3) (36 per 16)
        by the number of multiplies the feature map needs with each tiling - (m+2)^2 * ceil(H/m) * ceil(W/m): 9600 vs
        12420 per channel pair at 60x90, where 6 divides both sides, but F(4x4) wins on small maps with ragged 6x6
        tiles.  XL_WINOGRAD=4 / 2 forces F(4x4,3x3) / F(2x2,3x3) (the latter for inference only).  Training plans make the
        same choice, for the forward pass and for both gradients."""
        t, H, W, C, ld, off = act
        if (conv.kernel_size[0] != 3 or conv.stride[0] != 1 or C % 32 != 0 or H * W < 64
                or conv.out_channels not in (128, 256, 512, 1024) or self.sw.NO_WINOGRAD):
            return 0
        want = int(self.sw.WINOGRAD)
        if self.train and (self.sw.NO_WINOGRAD_TRAIN or want not in (4, 6)):
            return 0
        if want == 2:
            return 2 if not (H % 2 or W % 2) and self.B * (H // 2) * (W // 2) * max(C, conv.out_channels) * 4 < 2 ** 31 - 1 else 0
        return self.wino_pick(H, W, max(C, conv.out_channels))

    def wino_gemm_form(self, C, cout, m, T):
        """(split, split_il, split_act) of the GEMMs of an F(m x m,3x3) layer with T tiles.  XL_GEMM_SPLIT_BF16: "il" =
        interleaved planes + 256 x 256 persistent kernels, "1" = separate planes + 128 x 128 register-staged kernel (the
        first form), "0" = fp32 MFMA.  split_act (round 3): V stays fp32 in HBM (4 bytes per element instead of 6, written
        once and read once) and the GEMM kernel splits it on its way into LDS, like the activations of a 1x1 layer
        (XL_CONV_SPLIT_ACT); XL_WINO_V_SPLIT=1: the round-2 form, V written as interleaved bf16 planes by the input transform."""
        nf = (m + 2) ** 2
        mode = self.sw.GEMM_SPLIT_BF16
        split = (mode not in ("", "0") and C % 32 == 0 and self.split_train_ok())
        split_il = split and mode != "1" and (T + 256) * max(C * 6, cout * 4) < 2 ** 31 - 1 and C % 128 == 0 and cout % 256 == 0
        split_act = split_il and cout <= 1024 and not self.sw.WINO_V_SPLIT
        if m != 6 or self.train:
            # the forms that read V as bf16 planes exist for F(6x6,3x3) inference layers only (wino6_in_kernel writes them);
            # the form that splits an fp32 V inside the GEMM does not care about the tile size, and leaves V as the weight
            # gradient of a training plan wants it
            split = split_il = split_act
        if split and not split_il:
            split = nf * T * max(C, cout) * 6 < 2 ** 31 - 1             # (the first form addresses a plane as a whole)
        return split, split_il, split_act

    def fold_ok(self):
        return not self.train and not self.sw.NO_DEFERRED_GN and not self.sw.NO_FOLD_GN

    def stem12_ok(self, enc):
        """conv1 evaluated inside conv2's operand stage (csrc/xl_stem_fused.hip, round 4): inference plans whose stem runs on
        the split pipe.  A choice by layer, never by batch.  XL_NO_STEM12=1: the two-kernel path (conv1 writes its raw output,
        conv2 normalises and splits it on load)."""
        c2 = enc.conv2
        return (c2.in_channels == 32 and c2.out_channels == 64 and c2.kernel_size[0] == 3 and c2.stride[0] == 2
                and self.split_train_ok() and self.sw.split_on
                and not self.sw.NO_SPLIT_STEM and not self.sw.NO_STEM12
                and not self.sw.CONV1_VALU and not self.sw.NO_DEFERRED_GN)

    @staticmethod
    def _stem_stat_shape(cop, y):
        """(rows per tile, statistics entries per tile, nchunks) of a stride-2 stem convolution on the split pipe
        (csrc/xl_stem_split.hip: one fp64 entry per tile and row block of waves; include/crossloc_cnn.h)."""
        bm, wm = (128, 2) if cop.reserved_i == 128 else {64: (128, 4), 128: (128, 2), 256: (256, 2)}[y[3]]
        return bm, wm, (-(-(y[1] * y[2]) // bm) + 1) * wm

    def stem_stats_ok(self, norm, cout, train=False):
        """The stride-2 stem kernels (split pipe) sum the GroupNorm statistics of their output in the epilogue.
        Not for batch-invariant plans (the partial sums are grouped by tile, i.e. by the frame's position in the batch)."""
        return (self.train == train and not self.separate_stats and norm.num_groups == 32 and cout in (64, 128, 256)
                and not self.sw.STEM_FORM and not self.sw.NO_STEM_STATS)
