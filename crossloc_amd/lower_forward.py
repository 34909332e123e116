"""Forward lowering: a network and an input shape -> the op list of `_Plan.ops` (+ the tape a training plan's backward
lowering reads).  Mixed into `networks._Plan`."""
import torch

from .ops import (CONV_M_TILE_MAJOR, CONV_NORM_ADD, CONV_NORM_IN, CONV_NORM_RELU, CONV_PAIR_F16, CONV_SPLIT_ACT,
                  CONV_SPLIT_BF16, CONV_SPLIT_IL, GN_ADD, GN_RELU_IN, GN_RELU_OUT, XL_OP_CONV, XL_OP_CONV1,
                  XL_OP_DUC_HEAD, XL_OP_GN_APPLY, XL_OP_GN_FINAL, XL_OP_GN_STATS, XL_OP_HEAD, XL_OP_STEM12,
                  XL_OP_WINO_IN, XL_OP_WINO_OUT, XlOp, act_ptr)


class _Dummy:
    @staticmethod
    def data_ptr():
        return 0


_DUMMY = _Dummy()


class _ForwardLowering:
    # -- workspace
    def alloc(self, numel):
        lst = self.free.get(numel)
        if lst:
            return lst.pop()
        t = torch.empty(numel, dtype=torch.float32, device=self.device)
        self.keep.append(t)
        return t

    def release(self, t):
        if self.train:                      # training keeps every forward tensor for the backward pass
            return
        held = self.held.get(id(t))
        if held is not None:                # an input of a GroupNorm apply that a later op performs (fold): free it then
            held[1] = True
            return
        self.free.setdefault(t.numel(), []).append(t)

    # -- folded GroupNorm applies (inference plans).  A GroupNorm(+ReLU, +residual, +ReLU) whose result has SEVERAL consumers
    # - the first convolution of the next block and, later, a residual branch - used to be a pass of its own (read the raw
    # conv output and the residual, write the activation).  With `share` the pass is left to the first consumer when that is
    # an F(6x6,3x3) layer: its input transform reads the raw tensor and the residual anyway, applies the normalisation on load
    # and writes the activation (to a buffer of its own) for the consumers that follow.  Same arithmetic, same bits.
    def _fold_begin(self, ap, raw, aux):
        t, H, W, C, ld, off = raw
        mat = self.alloc(self.B * H * W * C)
        res = (mat, H, W, C, C, 0)
        tensors = [raw[0]] + ([aux[0]] if aux is not None else [])
        for x in tensors:
            self.held[id(x)] = [x, x is raw[0]]           # the raw conv output has no other owner: released with the fold
        self.pending_fold[self._act_key(res)] = dict(ap=ap, raw=raw, tensors=tensors, aux_ap=self._aux_take(aux))
        return res

    def _unhold(self, t):
        """End of a hold on a tensor (see `held`): release it now if its owner released it meanwhile."""
        if t is None:
            return
        entry = self.held.pop(id(t), None)
        if entry is not None and entry[1]:
            self.release(t)

    def _fold_end(self, fold):
        for x in fold["tensors"]:
            entry = self.held.pop(id(x))
            if entry[1]:
                self.release(x)

    def _fold_materialise(self, fold, act):
        """The first consumer cannot apply it on load: run the GroupNorm apply as a pass (raw -> the activation's buffer)."""
        ap = fold["ap"]
        ap.out, ap.ld_out = act_ptr(act), act[4]
        if fold.get("aux_ap") is not None:
            self._aux_apply(fold["aux_ap"])
        self.stats_ops.append(len(self.ops))
        self.ops.append(ap)
        self._fold_end(fold)

    # -- a residual whose own GroupNorm + ReLU has no other consumer than the addition (res2_conv3 -> res2_norm3 -> ReLU, added to
    # the normalised skip branch, networks.py:247-250 of the reference): its apply pass is left to the pass that performs the
    # addition - the fold form of the next block's input transform reads the RAW residual and normalises it while loading.  Its
    # {scale, shift} pairs must outlive the GN_FINAL of the skip branch: they go to a second coefficient table.
    def _aux_defer(self, act):
        """`act` was produced by cgr(..., defer=True): move its pending GroupNorm apply to the residual slot."""
        ap = self.pending_gn.pop(self._act_key(act), None)
        if ap is None:
            return                                    # (the layer's form could not defer it: it ran as a pass)
        assert not self.pending_aux
        fin = max(i for i, op in enumerate(self.ops) if op.type == XL_OP_GN_FINAL)
        self.aux_final_ops.append(fin)
        self.pending_aux = {self._act_key(act): ap}

    def _aux_take(self, aux):
        return self.pending_aux.pop(self._act_key(aux), None) if aux is not None else None

    def _emit_apply(self, ap, aux=None):
        """Emit a GroupNorm apply pass of an inference plan (it reads the shared statistics scratch) - behind the apply of its
        residual `aux`, if that one was left to it."""
        aux_ap = self._aux_take(aux)
        if aux_ap is not None:
            self._aux_apply(aux_ap)
        self.stats_ops.append(len(self.ops))
        self.ops.append(ap)

    def _aux_apply(self, ap):
        """The addition is not performed by a fold: apply the residual's GroupNorm as a pass after all (in place)."""
        self.aux_apply_ops.append(len(self.ops))
        self.stats_ops.append(len(self.ops))
        self.ops.append(ap)

    def release_grad(self, t):
        self.free.setdefault(t.numel(), []).append(t)

    # -- op emitters; an activation is (tensor, H, W, C, ld, channel_offset)

    def conv(self, act, conv, out=None, out_ld=None, out_off=0, norm_in=None, split=False):
        t, H, W, C, ld, off = act
        k, s = conv.kernel_size[0], conv.stride[0]
        cout = conv.out_channels
        Ho = (H + 2 * (k // 2) - k) // s + 1
        Wo = (W + 2 * (k // 2) - k) // s + 1
        if out is None:
            out = self.alloc(self.B * Ho * Wo * cout)
            out_ld = cout
        op = XlOp(type=XL_OP_CONV, B=self.B, Hi=H, Wi=W, Cin=C, Ho=Ho, Wo=Wo, Cout=cout, ksize=k, stride=s, ld_in=ld, ld_out=out_ld,
                  in_=act_ptr(act), out=out.data_ptr() + 4 * out_off)
        if not split:
            op.w = self.pack_conv(conv).data_ptr()
        op.bias = self.dev(conv.bias).data_ptr()
        # 64-row tiles when 128-row tiles would not even fill one wave of workgroups over the 256 CUs
        bn = 128 if cout % 128 == 0 else 64
        if -(-self.B * Ho * Wo // 128) * -(-cout // bn) <= 256 and norm_in is None:
            op.reserved_i = 64                        # (the normalise-on-load form exists with 128-row tiles only)
        if split and k == 3:                          # stride-2 stem layer on the split pipe (no statistics epilogue)
            op.flags |= CONV_SPLIT_BF16 | CONV_SPLIT_IL
            if (self.pair_ok() and (norm_in is not None or (self.train and self.sw.TRAIN_PAIR_STEM))
                    and not self.sw.NO_PAIR_STEM):
                # round 5: fp16 pairs, three passes (csrc/xl_stem_pair.hip); the operand is a GroupNorm output normalised on load.
                # Training plans (materialised GroupNorm + ReLU outputs: the same bound holds) run them too since round 6
                # (XL_TRAIN_PAIR_STEM=0: the six-pass kernels; -0.2 ms of a 32.4 ms step.  Round 5 left them off because one small-map
                # test counted ReLU-kink flips as errors: tests/test_semantics_gpu.py now uses the criterion of the other gradient tests)
                op.flags |= CONV_PAIR_F16
                op.w = self.pack_conv_stem_pair(conv).data_ptr()
                op.scale = self.pair_scales.data_ptr()
            else:
                op.w = self.pack_conv_stem_split(conv).data_ptr()
            op.reserved_i = 0
            if (cout == 256 and -(-self.B * Ho * Wo // 256) < 128 and not self.sw.NO_SMALL_TILES):
                op.reserved_i = 128                  # latency form: 128 x 128 tiles when 256-row tiles leave the chip idle
        elif split:
            op.flags |= CONV_SPLIT_BF16 | CONV_SPLIT_IL
            if self.pair_ok():
                # round 5: three fp16 passes instead of six bf16 ones; the operand is a GroupNorm output (or normalised on load)
                op.flags |= CONV_PAIR_F16
                op.w = self.pack_conv_1x1_pair(conv).data_ptr()
                op.scale = self.pair_scales.data_ptr()
            else:
                op.w = self.pack_conv_1x1_split(conv).data_ptr()
            # rows per tile (the statistics epilogue writes one entry per tile); negative: tiles start at image boundaries,
            # so the grouping of the partial sums does not depend on where a frame sits in the batch (batch-invariant plans)
            op.reserved_i = -256 if self.separate_stats else self.split_tile_form(self.B * Ho * Wo, cout, 1, Ho * Wo)
        if norm_in is not None:                       # the producer's deferred GroupNorm apply, folded into the operand load
            op.flags |= CONV_NORM_IN | (CONV_NORM_RELU if norm_in.flags & GN_RELU_IN else 0)
            if norm_in.flags & GN_ADD:                # ... + residual + ReLU (XL_CONV_NORM_ADD, split 1x1 kernel only)
                assert split and k == 1 and (norm_in.flags & GN_RELU_OUT) and (norm_in.flags & GN_RELU_IN)
                op.flags |= CONV_NORM_ADD
                op.aux, op.ld_aux = norm_in.aux, norm_in.ld_aux
            if self.train:
                op.aux2 = norm_in.aux2                # (training plans: the producer's own coefficient table)
            else:
                self.deferred_gn_consumers.append(len(self.ops))
        self.ops.append(op)
        res = (out, Ho, Wo, cout, out_ld, out_off)
        self.tape.append(dict(kind="conv", conv=conv, x=act, raw=res, xnorm=norm_in if self.train else None))
        return res

    def gn(self, act, norm, flags, aux=None, out=None, pre_stats=None, stat_tile=0, defer=False, share=False, stat_mult=1):
        """GroupNorm (+fused epilogue) of `act`; in place unless `out` (tensor, ld, off) is given or training.
        pre_stats = (stats tensor, nchunks): the partial sums were already produced (Winograd output transform or conv
        epilogue of a training plan; stat_tile = rows per conv tile in the latter case), no statistics pass is emitted.
        Training plans keep one coefficient table per layer ({scale, shift} and {mean, rstd} per image and channel,
        written by GN_FINAL): the apply pass and the three backward passes read it instead of re-reducing the partial
        sums in the prologue of every workgroup."""
        t, H, W, C, ld, off = act
        G = norm.num_groups
        HW = H * W
        nchunks = max(1, min(128, (HW + 255) // 256)) if pre_stats is None else pre_stats[1]
        st = XlOp(type=XL_OP_GN_STATS, B=self.B, Hi=H, Wi=W, Cin=C, groups=G, nchunks=nchunks, ld_in=ld, in_=act_ptr(act))
        ap, gamma, beta = self._gn_apply_op(act, norm, flags, nchunks, aux)
        stats_t = None
        if pre_stats is not None:
            assert self.train
            stats_t = pre_stats[0]
            ap.stats = stats_t.data_ptr()
        elif self.train:                    # the forward statistics are inputs of the backward pass: keep them
            stats_t = torch.zeros(self.B * nchunks * G * 2, dtype=torch.float64, device=self.device)
            self.keep.append(stats_t)
            st.stats = ap.stats = stats_t.data_ptr()
        else:
            self.max_stats = max(self.max_stats, self.B * nchunks * G * 2)
            self.stats_ops += [len(self.ops), len(self.ops) + 1]
        if pre_stats is None:
            self.ops.append(st)
        table = None
        if self.train:
            table = torch.zeros(self.B * C * 4, dtype=torch.float32, device=self.device)
            self.keep.append(table)
        self._emit_final(ap, gamma, beta, stat_tile, table, mult=stat_mult)
        # round 4, training plans: a GroupNorm + ReLU whose only consumer is a convolution that can apply it while loading its
        # operand (an F(m x m,3x3) layer: input transform, the normalised V is kept for the weight gradient; a 1x1 layer on the
        # split pipe: forward and weight-gradient kernels normalise on load) is NOT materialised: no apply pass, no activation
        # tensor.  Its backward pass needs the raw conv output and the coefficient table only.  cgr() materialises it after all
        # when the consumer turns out not to be able to (XL_NO_TRAIN_DEFER=1: never deferred).
        train_defer = (self.train and defer and out is None and flags == GN_RELU_IN and aux is None and not self.separate_stats
                       and HW % 8 == 0 and not self.sw.NO_TRAIN_DEFER)
        if out is None and self.train and not train_defer:
            out = (self.alloc(self.B * HW * C), C, 0)
        res = act if out is None else self._apply_into(ap, act, out)
        if not self.train and res is act:
            if defer:                                 # the only consumer applies it while loading its operand
                self.pending_gn[self._act_key(res)] = ap
                return res
            if share and self.fold_ok():              # ... or the first of several consumers does, and materialises it
                return self._fold_begin(ap, act, aux)
        if train_defer:
            entry = dict(kind="gn", norm=norm, raw=act, out=res, aux=None, flags=flags, table=table, gamma=gamma, beta=beta)
            self.tape.append(entry)
            self.pending_gn[self._act_key(res)] = ap
            self.pending_entry[self._act_key(res)] = entry
            return res
        aux_ap = self._aux_take(aux)
        if aux_ap is not None:
            self._aux_apply(aux_ap)
        self.ops.append(ap)
        self.tape.append(dict(kind="gn", norm=norm, raw=act, out=res, aux=aux, flags=flags, table=table,
                              gamma=gamma, beta=beta))
        return res

    def _gn_apply_op(self, act, norm, flags, nchunks, aux=None, tile=0):
        """The GN_APPLY op of `act` - in place until _apply_into() redirects it - and the layer's affine parameters on the device."""
        t, H, W, C, ld, off = act
        gamma, beta = self.dev(norm.weight), self.dev(norm.bias)
        ap = XlOp(type=XL_OP_GN_APPLY, B=self.B, Hi=H, Wi=W, Cin=C, groups=norm.num_groups, nchunks=nchunks, ld_in=ld, ld_out=ld,
                  flags=flags, eps=norm.eps, reserved_i=tile, in_=act_ptr(act), out=act_ptr(act), w=gamma.data_ptr(), bias=beta.data_ptr())
        if aux is not None:
            ap.aux, ap.ld_aux = act_ptr(aux), aux[4]
        return ap, gamma, beta

    @staticmethod
    def _apply_into(ap, act, out):
        """Point the apply op at `out` = (tensor, ld, channel offset); returns the activation it then writes."""
        ot, old, ooff = out
        ap.out, ap.ld_out = ot.data_ptr() + 4 * ooff, old
        return (ot, act[1], act[2], act[3], old, ooff)

    def _train_materialise(self, pend, act):
        """A GroupNorm apply deferred in a training plan whose consumer cannot apply it on load: run it as a pass into a buffer of
        its own (the raw conv output stays: the backward pass reads it) and continue with that activation."""
        t, H, W, C, ld, off = act
        out = self.alloc(self.B * H * W * C)
        pend.out, pend.ld_out = out.data_ptr(), C
        self.ops.append(pend)
        res = (out, H, W, C, C, 0)
        entry = self.pending_entry.pop(self._act_key(act), None)
        if entry is not None:
            entry["out"] = res
        return res

    def conv_wino(self, act, conv, norm, flags, aux, m, deferred=None, defer=False, fold=None, share=False, dst=None):
        """conv3x3 + GroupNorm(+epilogue) as F(m x m, 3x3): input transform, (m+2)^2 GEMMs in one batched launch, output
        transform that also emits the GroupNorm partial sums, GN_FINAL, GN_APPLY (in place; `dst` = (tensor, ld, channel
        offset): the apply writes the activation there instead - an encoder's last layer into its slice of the concat buffer)."""
        t, H, W, C, ld, off = act
        B, cout = self.B, conv.out_channels
        Th, Tw = -(-H // m), -(-W // m)
        T = B * Th * Tw
        nf = (m + 2) ** 2
        # the GEMMs on the bf16 matrix pipe with every fp32 operand split into three bf16 terms (fp32-accurate): wino_gemm_form
        split, split_il, split_act = self.wino_gemm_form(C, cout, m, T)
        assert fold is None or not split or split_act
        V = self.alloc(nf * T * C * 3 // 2 if (split and not split_act) else nf * T * C)
        op = XlOp(type=XL_OP_WINO_IN, ksize=m, B=B, Hi=H, Wi=W, Cin=C, Ho=Th, Wo=Tw, ld_in=ld, in_=act_ptr(act), out=V.data_ptr())
        # round 5: fp16 pairs (XL_CONV_PAIR_F16).  With full 256 x 256 tiles V is written as pairs by the input transform and both
        # operands of the GEMM arrive by DMA (pair_gemm_kernel); the small-batch tile forms keep V in fp32 and form the pairs in
        # the GEMM (pair_conv1x1_kernel with XL_CONV_SPLIT_ACT)
        pair = split_act and m == 6 and self.pair_ok()
        tile_form = self.split_tile_form(T, cout, nf) if split_act else 0
        # (training plans keep V in fp32: it is the left operand of the Winograd weight gradient)
        pair_dma = pair and tile_form == 256 and not self.train and not self.sw.PAIR_NO_DMA
        if pair_dma:
            op.flags = CONV_PAIR_F16
            op.scale = self.pair_scales.data_ptr() + 8
        if split and not split_act:
            op.flags = CONV_SPLIT_BF16 | (CONV_SPLIT_IL if split_il else 0)
        if deferred is not None:                      # the producer's GroupNorm(+ReLU) is applied while gathering
            op.flags |= deferred.flags
            if self.train:
                op.aux2 = deferred.aux2               # (training plans: the producer's own coefficient table)
            else:
                self.deferred_gn_consumers.append(len(self.ops))
        if fold is not None:                          # ... and, fold: the activation `act` is written by this transform
            fap, raw = fold["ap"], fold["raw"]
            op.in_, op.ld_in = act_ptr(raw), raw[4]
            op.flags |= fap.flags & (GN_RELU_IN | GN_ADD | GN_RELU_OUT)
            op.out2, op.ld_out = act_ptr(act), ld
            if fap.flags & GN_ADD:
                op.aux, op.ld_aux = fap.aux, fap.ld_aux
                if fold.get("aux_ap") is not None:    # the residual is a raw conv output: its {scale, shift} pairs in `w`
                    self.aux_coef_consumers.append(len(self.ops))
            self.deferred_gn_consumers.append(len(self.ops))
        self.ops.append(op)
        if fold is not None:
            self._fold_end(fold)
        Mb = self.alloc(nf * T * cout)
        op = XlOp(type=XL_OP_CONV, B=B, Hi=Th, Wi=Tw, Cin=C, Ho=Th, Wo=Tw, Cout=cout, ksize=1, stride=1, ld_in=C, ld_out=cout,
                  nchunks2=nf, in_=V.data_ptr(), out=Mb.data_ptr())
        # XL_WINO_M_TILE_MAJOR=1: the product M as [tiles][64][C], so that the block the output transform reads per tile is one
        # contiguous piece.  Measured at 47 frames: output transforms 3.21 -> 3.05 ms per step, GEMM epilogues +0.17 ms: no net
        # gain, so [64][tiles][C] (what every other form reads and writes) stays the default
        m_tile_major = CONV_M_TILE_MAJOR if (split_act and m == 6 and self.sw.WINO_M_TILE_MAJOR and not pair_dma) else 0
        if split:
            op.flags = (CONV_SPLIT_BF16 | (CONV_SPLIT_IL if split_il else 0) | (CONV_SPLIT_ACT if split_act else 0)
                        | m_tile_major)
            if pair:
                op.flags |= CONV_PAIR_F16
                if pair_dma:
                    op.flags &= ~CONV_SPLIT_ACT
                op.w = self.pack_conv_wino_pair(conv, m).data_ptr()
                op.scale = self.pair_scales.data_ptr() + 8
            else:
                op.w = self.pack_conv_wino_split(conv, m, split_il).data_ptr()
        else:
            op.w = self.pack_conv_wino(conv, m).data_ptr()
        if -(-T // 128) * (cout // 128) * nf <= 256:
            op.reserved_i = 64
        if split_act:
            op.reserved_i = tile_form
        self.ops.append(op)
        self.wino_gemm_indices.append(len(self.ops) - 1)
        self.release(V)
        out = self.alloc(B * H * W * cout)
        G = norm.num_groups
        tpb = self.wino_out_tpb(m, Th * Tw, cout)
        if self.sw.WINO_OUT_TPB:
            tpb = int(self.sw.WINO_OUT_TPB)
        if self.separate_stats:
            tpb = 4          # batch-invariant plans: the grouping of the partial sums must not depend on the batch size
        nchunks = -(-(Th * Tw) // tpb)
        op = XlOp(type=XL_OP_WINO_OUT, ksize=m, B=B, Hi=H, Wi=W, Cin=cout, ld_out=cout, groups=G, nchunks=nchunks, reserved_i=tpb,
                  flags=m_tile_major, in_=Mb.data_ptr(), out=out.data_ptr(), bias=self.dev(conv.bias).data_ptr())
        y = (out, H, W, cout, cout, 0)
        if self.train:
            # the raw conv output and its statistics are inputs of the backward pass: keep both, record the tape
            stats_t = torch.zeros(B * nchunks * G * 2, dtype=torch.float64, device=self.device)
            self.keep.append(stats_t)
            op.stats = stats_t.data_ptr()
            self.ops.append(op)
            self.free.setdefault(Mb.numel(), []).append(Mb)          # M is scratch even in training plans
            # V = B^T x B is also the left operand of the Winograd weight gradient: keep it (407 MB per 512-channel
            # layer at batch 16) instead of transforming the input again, within a fixed budget
            kept_v = None
            if (m in (4, 6) and conv.weight.requires_grad and self.kept_v_bytes + 4 * V.numel() <= (16 << 30)
                    and not self.sw.NO_KEEP_V and not self.sw.NO_WINOGRAD_WGRAD):
                kept_v = V
                self.kept_v_bytes += 4 * V.numel()
            else:
                self.free.setdefault(V.numel(), []).append(V)
            self.tape.append(dict(kind="conv", conv=conv, x=act, raw=y, v=kept_v, wm=m, xnorm=deferred))
            return self.gn(y, norm, flags, aux, pre_stats=(stats_t, nchunks), out=dst, defer=defer)
        self.max_stats = max(self.max_stats, B * nchunks * G * 2)
        self.stats_ops.append(len(self.ops))
        self.ops.append(op)
        self.release(Mb)
        ap, gamma, beta = self._gn_apply_op(y, norm, flags, nchunks, aux)
        self._emit_final(ap, gamma, beta, 0)
        if dst is not None:                            # the apply is a pass of its own: raw conv output -> the destination slice
            res = self._apply_into(ap, y, dst)
            self._emit_apply(ap, aux)
            self.release(out)
            return res
        if defer and flags == GN_RELU_IN and aux is None and not self.sw.NO_DEFERRED_GN:
            # the only consumer applies it while loading its operand (a 1x1 conv: norm_on_load_ok; or a Winograd transform)
            self.pending_gn[self._act_key(y)] = ap
            return y
        if share and self.fold_ok():
            return self._fold_begin(ap, y, aux)
        self._emit_apply(ap, aux)
        return y

    def cgr(self, act, conv, norm, flags=GN_RELU_IN, aux=None, defer=False, share=False, out=None, defer_add=False):
        """conv -> GroupNorm -> epilogue.  `defer`: the caller promises that the next cgr() is the only consumer of the
        result; when that consumer is an F(4x4,3x3) layer its input transform applies the normalisation and the separate
        GN_APPLY pass (one read + one write of the activation) disappears.  `out` = (tensor, ld, channel offset): the
        activation is written there (an encoder's last layer into its slice of the MLR concat buffer)."""
        pend = self.pending_gn.pop(self._act_key(act), None)
        fold = self.pending_fold.pop(self._act_key(act), None)
        m = self.wino_tile(act, conv)
        if out is not None and not m:                  # no Winograd form for this layer: direct conv, then the apply into `out`
            if pend is not None and self.train:
                act = self._train_materialise(pend, act)
            elif pend is not None:
                self._emit_apply(pend)
            if fold is not None:
                self._fold_materialise(fold, act)
            y = self.conv(act, conv)
            r = self.gn(y, norm, flags, aux, out=out)
            if r[0] is not y[0]:
                self.release(y[0])
            return r
        stem = self.stem_split_ok(act, conv)
        cpg = conv.out_channels // norm.num_groups
        # a 1x1 layer on the split pipe applies a pending GroupNorm on load at ANY batch size (the tile-count condition of
        # norm_on_load_ok belongs to the fp32 kernel's 64-row form)
        # (the statistics epilogue of the split kernel sums 16-channel groups; a layer with other groups - res1_conv2: 8 per
        #  group - still runs on the split pipe in inference plans, followed by a statistics pass over its output)
        split_1x1 = self.split_1x1_ok(act, conv) and (cpg == 16 or self.separate_stats or not self.train)
        absorbs = (split_1x1 and act[3] <= 512 and act[1] * act[2] >= 256 and not self.sw.NO_NORM_ON_LOAD)
        if pend is not None and self.train:
            # training plans: absorbed by a Winograd layer (V is kept normalised) or by a 1x1 layer whose forward AND
            # weight-gradient kernels normalise on load; anything else gets the activation materialised
            t_ok = (m in (4, 6) and self.wino_wgrad_ok(conv, act[1], act[2], act[3], m)) or \
                   (split_1x1 and absorbs and cpg == 16 and self.wgrad_split_ok(act[3], conv.out_channels)
                    and act[4] % 4 == 0 and act[5] % 4 == 0)
            if not t_ok:
                act = self._train_materialise(pend, act)
                pend = None
            else:
                self.pending_entry.pop(self._act_key(act), None)
        pend_add = pend is not None and bool(pend.flags & GN_ADD)
        if pend is not None and not self.train and ((m not in (4, 6) and not self.norm_on_load_ok(act, conv) and not stem and not absorbs)
                                                    or (pend_add and not absorbs)):
            self._emit_apply(pend)       # consumer cannot absorb it: materialise now
            pend = None
        held_res = None
        if pend_add:                                   # the residual is dead once the consumer (or the apply pass) is emitted
            held_res = self.pending_res.pop(self._act_key(act), None)
            if pend is None:                           # (materialised just above)
                self._unhold(held_res)
                held_res = None
        if fold is not None:
            # the fold form of the input transform writes V as fp32 (F(6x6,3x3) layers whose GEMMs read fp32 activations)
            tiles6 = self.B * -(-act[1] // 6) * -(-act[2] // 6)
            sp, _, sp_act = self.wino_gemm_form(act[3], conv.out_channels, m, tiles6) if m == 6 else (0, 0, 0)
            if m != 6 or (sp and not sp_act):
                self._fold_materialise(fold, act)
                fold = None
        if m:
            return self.conv_wino(act, conv, norm, flags, aux, m, pend, defer=defer, fold=fold, share=share, dst=out)
        dfr = defer and flags == GN_RELU_IN and aux is None and not self.sw.NO_DEFERRED_GN
        if stem:
            # conv on the split pipe with the producer's GroupNorm applied on load; statistics pass; the apply is left to the
            # consumer (the next stem layer, or - conv4 - the input transform of res1_conv1)
            y = self.conv(act, conv, norm_in=pend, split=True)
            if self.stem_stats_ok(norm, conv.out_channels):
                # round 4: the statistics come from the convolution's epilogue (one entry per tile and row block of waves)
                bm, wm, nchunks = self._stem_stat_shape(self.ops[-1], y)
                return self.gn_fused(y, norm, flags, aux, len(self.ops) - 1, defer=dfr, share=share, stat=(bm, wm, nchunks))
            if self.train and self.sw.TRAIN_STEM_STATS and self.stem_stats_ok(norm, conv.out_channels, train=True):
                # training (opt-in, XL_TRAIN_STEM_STATS=1): the same epilogue statistics in a buffer of the layer's own (GN_FINAL
                # turns them into the table the apply and the backward passes read).  Not the default: the step time does not
                # move (40.5 ms either way, three 47 us passes) and the fp32 trees perturb the statistics by ~1e-7, which is
                # enough to flip ReLUs at the kinks and move the small-map gradient test against float64 autograd
                # (tests/test_semantics_gpu.py) from 0.047 to 0.063 of the max-norm
                bm, wm, nchunks = self._stem_stat_shape(self.ops[-1], y)
                return self.gn(y, norm, flags, aux, pre_stats=self._own_stats(self.ops[-1], norm, nchunks), stat_tile=bm, stat_mult=wm,
                               defer=dfr)
            return self.gn(y, norm, flags, aux, defer=dfr, share=share)
        split = split_1x1 and (pend is None or absorbs)
        y = self.conv(act, conv, norm_in=pend, split=split)
        self._unhold(held_res)
        bn = 128 if conv.out_channels % 128 == 0 else 64
        # a conv tile's columns cover whole groups, and the statistics epilogue sums 2- or 4-channel pieces
        whole_groups = bn % cpg == 0 and (cpg == 2 or cpg % 4 == 0)
        if (not self.train and y[1] * y[2] >= 128 and whole_groups and (not split or cpg == 16)
                and (not self.separate_stats or (split and cpg == 16))):
            # inference: the conv epilogue produces the GroupNorm statistics, the separate stats pass is dropped
            # defer_add (round 4): the caller promises that the only consumer is a 1x1 layer on the split pipe - it applies the whole
            # GroupNorm + ReLU + residual + ReLU epilogue while it loads its operand (XL_CONV_NORM_ADD), no apply pass
            add_on_load = (defer_add and flags == (GN_RELU_IN | GN_ADD | GN_RELU_OUT) and aux is not None and split
                           and not self.sw.NO_DEFERRED_GN and not self.sw.NO_ADD_ON_LOAD)
            return self.gn_fused(y, norm, flags, aux, len(self.ops) - 1, defer=dfr or add_on_load, share=share)
        if (self.train and y[1] * y[2] >= 128 and whole_groups and not self.separate_stats
                and self.ops[-1].type == XL_OP_CONV):
            # training: the same epilogue statistics
            tile = 64 if self.ops[-1].reserved_i == 64 else (256 if split else 128)
            stats = self._own_stats(self.ops[-1], norm, (y[1] * y[2] + tile - 1) // tile + 1)
            return self.gn(y, norm, flags, aux, pre_stats=stats, stat_tile=tile, defer=defer)
        if not self.train:
            return self.gn(y, norm, flags, aux, defer=dfr, share=share)
        r = self.gn(y, norm, flags, aux, defer=defer)
        if r[0] is not y[0]:
            self.release(y[0])
        return r

    def _own_stats(self, cop, norm, nchunks):
        """Training plans: the conv op `cop` writes the GroupNorm statistics of its epilogue to a buffer of the layer's own - they
        are inputs of the backward pass.  Slots a conv tile never touches stay zero, so the consumers may sum all of them.
        Returns gn()'s `pre_stats`."""
        stats_t = torch.zeros(self.B * nchunks * norm.num_groups * 2, dtype=torch.float64, device=self.device)
        self.keep.append(stats_t)
        cop.stats, cop.groups, cop.nchunks = stats_t.data_ptr(), norm.num_groups, nchunks
        return stats_t, nchunks

    @staticmethod
    def _act_key(act):
        return (act[0].data_ptr(), act[5], act[3])

    def gn_fused(self, act, norm, flags, aux, conv_index, out=None, defer=False, share=False, stat=None):
        """GroupNorm apply (in place) consuming statistics emitted by the epilogue of the conv op `conv_index`.
        stat = (rows per tile, entries per tile, nchunks) when the producer is not the 1x1 / direct kernel (the stride-2 stem
        kernels: one entry per tile and row block of waves; rows per tile 0: all nchunks entries are written)."""
        t, H, W, C, ld, off = act
        G, HW = norm.num_groups, H * W
        cop = self.ops[conv_index]
        mult = 1
        if stat is not None:
            tile, mult, nchunks = stat
        else:
            tile = cop.reserved_i if cop.reserved_i in (64, 256, -256) else (256 if cop.reserved_i in (192, 384) else 128)
            nchunks = (HW + abs(tile) - 1) // abs(tile) + 1
        self.max_stats = max(self.max_stats, self.B * nchunks * G * 2)
        cop.groups, cop.nchunks = G, nchunks
        ap, gamma, beta = self._gn_apply_op(act, norm, flags, nchunks, aux, tile=tile)
        self.stats_ops.append(conv_index)
        self._emit_final(ap, gamma, beta, tile, mult=mult)
        res = act if out is None else self._apply_into(ap, act, out)
        if defer and out is None:
            self.pending_gn[self._act_key(res)] = ap
            if aux is not None:                        # (the residual must outlive the caller's release until the consumer is emitted)
                self.held[id(aux[0])] = [aux[0], False]
                self.pending_res[self._act_key(res)] = aux[0]
            return res
        if share and out is None and self.fold_ok():
            return self._fold_begin(ap, act, aux)
        self._emit_apply(ap, aux)
        return res

    def _emit_final(self, ap, gamma, beta, stat_tile, table=None, mult=1):
        """GN_FINAL op: one tiny launch turns the partial sums into per-(image, channel) scale/shift so the
        streaming apply kernel does no redundant reduction per workgroup.  Inference: shared statistics and
        coefficient buffers, patched in once their sizes are known.  Training (`table`): the layer's own statistics
        (ap.stats) and its own table, {scale, shift} pairs first, {mean, rstd} pairs behind them."""
        fin = XlOp(type=XL_OP_GN_FINAL, B=ap.B, Hi=ap.Hi, Wi=ap.Wi, Cin=ap.Cin, groups=ap.groups, nchunks=ap.nchunks,
                   eps=ap.eps, reserved_i=stat_tile, stride=mult, w=gamma.data_ptr(), bias=beta.data_ptr())
        if table is None:
            self.max_coeff = max(self.max_coeff, self.B * ap.Cin * 2)
            self.stats_ops.append(len(self.ops))
        else:
            fin.stats = ap.stats
            fin.out, fin.out2 = table.data_ptr(), table.data_ptr() + 4 * self.B * ap.Cin * 2
            ap.aux2 = table.data_ptr()
        self.ops.append(fin)

    def res_block(self, res, block):
        """relu(res + block(res)), networks.py:252-254 / :332-334"""
        x = self.cgr(res, block[0], block[1], defer=True)
        x2 = self.cgr(x, block[3], block[4], defer=True)
        self.release(x[0])
        x3 = self.cgr(x2, block[6], block[7], GN_RELU_IN | GN_ADD | GN_RELU_OUT, aux=res, share=True)
        self.release(x2[0])
        self.release(res[0])
        return x3

    def encoder(self, enc, image, out=None):
        """networks.py:221-256.  `out` = (tensor, ld, off): write the final activation into a channel slice."""
        B, H, W = self.B, self.H, self.W
        tape_start = len(self.tape)
        frozen = not any(p.requires_grad for p in enc.parameters())
        try:
            return self._encoder_body(enc, image, out)
        finally:
            if frozen:
                for e in self.tape[tape_start:]:
                    e["frozen"] = True

    def _encoder_body(self, enc, image, out=None):
        B, H, W = self.B, self.H, self.W
        cin = enc.conv1.in_channels
        c1 = enc.conv1.out_channels
        if not self.train and cin == 3 and c1 == 32 and enc.norm1.num_groups == 32 and not self.sw.NO_CONV1_FUSED:
            if self.stem12_ok(enc):
                return self._encoder_tail(enc, None, out, x2=self._stem12(enc, image))
            x = self._conv1_fused(enc, image, self.alloc(B * H * W * c1))
            return self._encoder_tail(enc, x, out)
        t1 = self.alloc(B * H * W * c1)
        raw1, pre_stats = (t1, H, W, c1, c1, 0), None
        if (self.train and cin == 3 and c1 == 32 and enc.norm1.num_groups == 32 and self.split_train_ok() and self.sw.split_on
                and not self.sw.CONV1_VALU):
            # round 4, training plans: the matrix-pipe form of the inference plans, ONE evaluation that writes the raw output
            # (kept for the backward pass) together with its GroupNorm partial sums - no separate statistics pass over the
            # largest tensor of the network (conv1_direct_kernel + gn_stats: 0.52 + 0.13 ms at batch 16; this: 0.25)
            G = enc.norm1.num_groups
            nchunks = -(-H // 16) * -(-W // 64)
            stats_t = torch.zeros(B * nchunks * G * 2, dtype=torch.float64, device=self.device)
            self.keep.append(stats_t)
            op = self._conv1_op(enc, image, self.pack_conv1_split(enc.conv1), self.dev(enc.conv1.bias), groups=G, nchunks=nchunks,
                                eps=enc.norm1.eps, out=t1.data_ptr(), stats=stats_t.data_ptr())
            pre_stats = (stats_t, nchunks)
        else:
            op = self._conv1_op(enc, image, self.pack_conv(enc.conv1), self.dev(enc.conv1.bias), cin=cin, out=t1.data_ptr())
        self.image_op_indices.append(len(self.ops))
        self.ops.append(op)
        self.tape.append(dict(kind="conv1", conv=enc.conv1, raw=raw1))
        return self._encoder_tail(enc, self.gn(raw1, enc.norm1, GN_RELU_IN, pre_stats=pre_stats), out)

    def _conv1_op(self, enc, image, w, bias, cin=3, **fields):
        """An XL_OP_CONV1 over the image (whose address is patched in per call: the caller lists the op in image_op_indices).
        With groups / nchunks / eps the kernel also sums the GroupNorm statistics of its result; reserved_i = pixels per
        thread of the vector-ALU form, 0 = matrix pipe."""
        c1 = enc.conv1.out_channels
        return XlOp(type=XL_OP_CONV1, B=self.B, Hi=self.H, Wi=self.W, Cin=cin, Ho=self.H, Wo=self.W, Cout=c1, ld_out=c1,
                    in_=image.data_ptr(), w=w.data_ptr(), bias=bias.data_ptr(), **fields)

    def _stem12(self, enc, image):
        """conv1 statistics (one evaluation of conv1, nothing written), GN_FINAL, then the fused kernel: raw conv2 output.  The
        32-channel full-resolution activation (2 GB at 47 frames) is never allocated.  Returns conv2's GroupNorm'ed activation
        with its apply left to the consumer (conv3 on the split pipe)."""
        B, H, W = self.B, self.H, self.W
        c1, G = enc.conv1.out_channels, enc.norm1.num_groups
        nchunks = -(-H // 16) * -(-W // 64)
        w1, b1 = self.pack_conv1_split(enc.conv1), self.dev(enc.conv1.bias)
        gamma, beta = self.dev(enc.norm1.weight), self.dev(enc.norm1.bias)
        st = self._conv1_op(enc, image, w1, b1, groups=G, nchunks=nchunks, eps=enc.norm1.eps)
        self.max_stats = max(self.max_stats, B * nchunks * G * 2)
        self.stats_ops.append(len(self.ops))
        self.image_op_indices.append(len(self.ops))
        self.ops.append(st)
        shape = XlOp(B=B, Hi=H, Wi=W, Cin=c1, groups=G, nchunks=nchunks, eps=enc.norm1.eps)   # GN_FINAL sees the normalised tensor
        self._emit_final(shape, gamma, beta, 0)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        c2 = enc.conv2.out_channels
        y = self.alloc(B * Ho * Wo * c2)
        op = XlOp(type=XL_OP_STEM12, B=B, Hi=H, Wi=W, Cin=3, Ho=Ho, Wo=Wo, Cout=c2, ld_out=c2, ksize=3, stride=2, flags=GN_RELU_IN,
                  in_=image.data_ptr(), w=w1.data_ptr(), bias=b1.data_ptr(), out=y.data_ptr())
        if self.pair_ok() and not self.sw.NO_PAIR_STEM:
            # round 5: conv2 inside the fused kernel as three fp16 passes (conv1's normalised output is a GroupNorm output)
            op.flags |= CONV_PAIR_F16
            op.aux = self.pack_conv2_pair_fragments(enc.conv2).data_ptr()
            op.scale = self.pair_scales.data_ptr()
        else:
            op.aux = self.pack_conv2_fragments(enc.conv2).data_ptr()
        op.stats2 = self.dev(enc.conv2.bias).data_ptr()
        queue = torch.zeros(4, dtype=torch.int32, device=self.device)      # the launch's tile queue (zero before and after)
        self.keep.append(queue)
        op.out2 = queue.data_ptr()
        self.deferred_gn_consumers.append(len(self.ops))
        self.image_op_indices.append(len(self.ops))
        self.ops.append(op)
        raw2 = (y, Ho, Wo, c2, c2, 0)
        if self.stem_stats_ok(enc.norm2, c2) and enc.norm2.num_groups == 32:   # conv2's statistics from the fused kernel's epilogue
            th = 8 if self.sw.STEM12_TILE == "8" else 4
            return self.gn_fused(raw2, enc.norm2, GN_RELU_IN, None, len(self.ops) - 1, defer=not self.sw.NO_DEFERRED_GN,
                                 stat=(0, 1, -(-Wo // 16) * -(-Ho // th) * (th // 2)))
        return self.gn(raw2, enc.norm2, GN_RELU_IN, None, defer=not self.sw.NO_DEFERRED_GN)

    def _conv1_fused(self, enc, image, t1):
        """Inference form of conv1 + GroupNorm + ReLU: a statistics-only evaluation of the convolution, GN_FINAL, then
        a second evaluation that writes the normalised activation - the raw 32-channel full-resolution tensor (the
        largest of the network) is never written, re-read for statistics or re-read for the apply."""
        B, H, W = self.B, self.H, self.W
        c1, G, ppt = enc.conv1.out_channels, enc.norm1.num_groups, 5
        nchunks = -(-(H * W) // (256 * ppt))
        w, bias = self.pack_conv(enc.conv1), self.dev(enc.conv1.bias)
        if not self.sw.CONV1_VALU:       # matrix-pipe form: one workgroup per 16 x 64 output tile
            ppt, nchunks = 0, -(-H // 16) * -(-W // 64)
            w = self.pack_conv1_split(enc.conv1)
        st = self._conv1_op(enc, image, w, bias, groups=G, nchunks=nchunks, reserved_i=ppt, eps=enc.norm1.eps)
        self.max_stats = max(self.max_stats, B * nchunks * G * 2)
        act1 = (t1, H, W, c1, c1, 0)
        self.stats_ops.append(len(self.ops))
        self.image_op_indices.append(len(self.ops))
        self.ops.append(st)
        if ppt == 0 and self.stem_split_ok(act1, enc.conv2) and not self.sw.NO_DEFERRED_GN and not self.sw.CONV1_TWO_PASS:
            # round 3: ONE evaluation - the raw convolution is written together with its statistics, and conv2 (on the split
            # pipe) applies GroupNorm + ReLU while it gathers its operand: the statistics-only evaluation disappears
            st.out = t1.data_ptr()
            # the apply pass, left to the consumer (materialised only if it cannot)
            ap, gamma, beta = self._gn_apply_op(act1, enc.norm1, GN_RELU_IN, nchunks)
            self._emit_final(ap, gamma, beta, 0)
            self.pending_gn[self._act_key(act1)] = ap
            return act1
        shape = XlOp(B=B, Hi=H, Wi=W, Cin=c1, groups=G, nchunks=nchunks, eps=enc.norm1.eps)   # GN_FINAL sees the normalised tensor
        self._emit_final(shape, self.dev(enc.norm1.weight), self.dev(enc.norm1.bias), 0)
        ap = self._conv1_op(enc, image, w, bias, groups=G, nchunks=nchunks, reserved_i=ppt, eps=enc.norm1.eps,
                            out=t1.data_ptr(), flags=GN_RELU_IN)
        self.deferred_gn_consumers.append(len(self.ops))
        self.image_op_indices.append(len(self.ops))
        self.ops.append(ap)
        return act1

    def _encoder_tail(self, enc, x, out=None, x2=None):
        if x2 is None:
            x2 = self.cgr(x, enc.conv2, enc.norm2, defer=True); self.release(x[0])
        x3 = self.cgr(x2, enc.conv3, enc.norm3, defer=True); self.release(x2[0])
        res = self.cgr(x3, enc.conv4, enc.norm4, share=True); self.release(x3[0])
        a = self.cgr(res, enc.res1_conv1, enc.res1_norm1, defer=True)
        b = self.cgr(a, enc.res1_conv2, enc.res1_norm2, defer=True); self.release(a[0])
        c = self.cgr(b, enc.res1_conv3, enc.res1_norm3, GN_RELU_IN | GN_ADD | GN_RELU_OUT, aux=res, share=True)
        self.release(b[0]); self.release(res[0])
        res = c
        a = self.cgr(res, enc.res2_conv1, enc.res2_norm1, defer=True)
        b = self.cgr(a, enc.res2_conv2, enc.res2_norm2, defer=True); self.release(a[0])
        n_add = len(enc.enc_add_res_block_ls)
        last_out = out if n_add == 0 else None
        # (c is consumed by the addition below only: when that addition is folded into the next block's input transform, so is
        #  c's own GroupNorm + ReLU)
        aux_fold = last_out is None and self.fold_ok() and not self.sw.NO_AUX_FOLD
        if enc.tiny:
            # networks.py:245-250 with tiny=True: no projection on the skip path - res2 closes like res1, relu(res + x)
            c = self.cgr(b, enc.res2_conv3, enc.res2_norm3, GN_RELU_IN | GN_ADD | GN_RELU_OUT, aux=res,
                         share=last_out is None, out=last_out)
            self.release(b[0]); self.release(res[0])
            res = c
            return self._encoder_add_blocks(enc, res, out)
        c = self.cgr(b, enc.res2_conv3, enc.res2_norm3, defer=aux_fold); self.release(b[0])
        if aux_fold:
            self._aux_defer(c)
        if last_out is None:                        # conv -> GroupNorm with the statistics out of the conv epilogue
            skip_in = res
            res = self.cgr(skip_in, enc.res2_skip, enc.res2_skip_norm, GN_ADD | GN_RELU_OUT, aux=c, share=True)
            self.release(skip_in[0]); self.release(c[0])
        else:
            sk = self.conv(res, enc.res2_skip)
            self.release(res[0])
            res = self.gn(sk, enc.res2_skip_norm, GN_ADD | GN_RELU_OUT, aux=c, out=last_out)
            self.release(c[0])
            if res[0] is not sk[0]:
                self.release(sk[0])
        return self._encoder_add_blocks(enc, res, out)

    def _encoder_add_blocks(self, enc, res, out=None):
        """networks.py:252-254: the encoder's additional residual blocks; the last one writes into `out` if given."""
        n_add = len(enc.enc_add_res_block_ls)
        for i, block in enumerate(enc.enc_add_res_block_ls):
            if i == n_add - 1 and out is not None:
                # (round 4: like every other block - GroupNorm applies deferred to the consumer, the last 3x3 layer as
                #  Winograd - except that the block's final apply writes into the encoder's slice of the concat buffer.
                #  Until round 3 this block ran undeferred and its last layer as the DIRECT fp32-MFMA convolution: 4.3 ms
                #  instead of 0.9 per encoder at 24 frames)
                if self.sw.MLR_LAST_DIRECT:          # the round-3 lowering, kept for the A/B
                    x = self.cgr(res, block[0], block[1])
                    x2 = self.cgr(x, block[3], block[4]); self.release(x[0])
                    y = self.conv(x2, block[6]); self.release(x2[0])
                    r = self.gn(y, block[7], GN_RELU_IN | GN_ADD | GN_RELU_OUT, aux=res, out=out)
                    self.release(y[0]); self.release(res[0])
                    res = r
                    continue
                x = self.cgr(res, block[0], block[1], defer=True)
                x2 = self.cgr(x, block[3], block[4], defer=True); self.release(x[0])
                r = self.cgr(x2, block[6], block[7], GN_RELU_IN | GN_ADD | GN_RELU_OUT, aux=res, out=out)
                self.release(x2[0]); self.release(res[0])
                res = r
            else:
                res = self.res_block(res, block)
        return res

    def _lower(self, net):
        dec = net.decoder
        if net.num_mlr == 0:
            res = self.encoder(net.encoder, _DUMMY)
        else:
            c = (512, 128)[net.tiny]
            # encoders write straight into channel slices of the concat buffer (networks.py:485-488)
            h, w = self.H, self.W
            for _ in range(3):
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            Ho, Wo = h, w
            ctot = c * net.num_mlr
            cat = self.alloc(self.B * Ho * Wo * ctot)
            for i, enc in enumerate(net.mlr_encoder_ls):
                self.encoder(enc, _DUMMY, out=(cat, ctot, i * c))
            mlr = (cat, Ho, Wo, ctot, ctot, 0)
            sk = self.cgr(mlr, net.mlr_skip[0], net.mlr_skip[1], 0)
            # (mlr_norm's only consumer is the fusion layer: its input transform applies the normalisation - no apply pass over
            #  the 1536-channel buffer)
            mlr = self.gn(mlr, net.mlr_norm, 0, defer=not self.sw.NO_DEFERRED_GN)
            f = net.mlr_forward
            a = self.cgr(mlr, f[0], f[1], defer=True); self.release(cat)
            b = self.cgr(a, f[3], f[4], defer=True); self.release(a[0])
            res = self.cgr(b, f[6], f[7], GN_RELU_IN | GN_ADD | GN_RELU_OUT, aux=sk, share=True)
            self.release(b[0]); self.release(sk[0])
        for block in dec.dec_add_res_block_ls:
            res = self.res_block(res, block)
        a = self.cgr(res, dec.res3_conv1, dec.res3_norm1, defer=True)
        b = self.cgr(a, dec.res3_conv2, dec.res3_norm2, defer=True); self.release(a[0])
        # (res3's output has ONE consumer, fc1 - a 1x1 layer: its GroupNorm + ReLU + residual + ReLU is applied by fc1's operand load)
        c = self.cgr(b, dec.res3_conv3, dec.res3_norm3, GN_RELU_IN | GN_ADD | GN_RELU_OUT, aux=res, defer_add=True)
        self.release(b[0]); self.release(res[0])
        res = c
        a = self.cgr(res, dec.fc1, dec.fc1_norm, defer=True); self.release(res[0])
        b = self.cgr(a, dec.fc2, dec.fc2_norm, defer=True); self.release(a[0])
        if dec.full_size_output:
            # networks.py:344-349: DUC conv-GN-ReLU; pixel shuffle, bilinear trim and fc3 fused in one kernel
            d = self.cgr(b, dec.duc_upsample.conv, dec.duc_upsample.norm); self.release(b[0])
            self._head("duc_head", XL_OP_DUC_HEAD, dec, d, self.H, self.W)
            return
        pend = self.pending_gn.pop(self._act_key(b), None)
        if pend is not None and self.train:              # (the head's backward pass reads the normalised activation)
            b = self._train_materialise(pend, b)
            pend = None
        if pend is not None and not (b[3] == 512 and dec.num_task_channel + dec.num_pos_channel <= 4):
            self._emit_apply(pend)       # the general head form reads a normalised activation
            pend = None
        self._head("head", XL_OP_HEAD, dec, b, b[1], b[2], pend)

    def _head(self, kind, typ, dec, act, Ho, Wo, pend=None):
        """The plan's last op: fc3 and the coordinate epilogue on the decoder's last activation (XL_OP_HEAD; `pend`: fc2's
        GroupNorm + ReLU applied while it loads), or behind the pixel shuffle and bilinear trim of the DUC (XL_OP_DUC_HEAD)."""
        t, H, W, C, ld, off = act
        nout = dec.num_task_channel + dec.num_pos_channel
        w3 = dec.fc3.weight.detach().to(device=self.device, dtype=torch.float32).reshape(nout, -1).contiguous()
        self.keep.append(w3)
        op = XlOp(type=typ, B=self.B, Hi=H, Wi=W, Cin=C, Ho=Ho, Wo=Wo, Cout=nout,
                  n_task=dec.num_task_channel, n_pos=dec.num_pos_channel, ld_in=ld, clamp_lo=-16.10, clamp_hi=13.82,
                  in_=act_ptr(act), w=w3.data_ptr(), bias=self.dev(dec.fc3.bias).data_ptr(), aux=self.dev(dec.mean).data_ptr())
        if pend is not None:
            op.flags = CONV_NORM_RELU if pend.flags & GN_RELU_IN else 0
            self.deferred_gn_consumers.append(len(self.ops))
        self.ops.append(op)
        self.out_op_index = len(self.ops) - 1
        self.out_shape = (self.B, nout, Ho, Wo)
        self.tape.append(dict(kind=kind, fc3=dec.fc3, x=act, w3=w3, cout=nout, n_task=op.n_task))
