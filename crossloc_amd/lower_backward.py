"""Backward lowering of a training plan: the tape the forward lowering recorded, walked in reverse -> `_Plan.bwd_array`
(head backward, GroupNorm / epilogue backward, weight gradients, data gradients).  Mixed into `networks._Plan`."""
import numpy as np
import torch

from .ops import (CONV_ACCUMULATE, CONV_DGRAD, CONV_M_TILE_MAJOR, CONV_NORM_IN, CONV_NORM_RELU, CONV_PAIR_AMAX,
                  CONV_PAIR_F16, CONV_SPLIT_ACT, CONV_SPLIT_BF16, CONV_SPLIT_IL, GNB_PARAMS_ITEM_DTYPE, GN_ACC_AUX,
                  GN_ADD, GN_NO_CONV_BIAS, GN_RELU_IN, GN_RELU_OUT, XL_OP_CONV, XL_OP_CONV1_WGRAD, XL_OP_DUC_HEAD_BWD,
                  XL_OP_FILL0, XL_OP_GNB_APPLY, XL_OP_GNB_FINAL, XL_OP_GNB_PARAMS, XL_OP_GNB_PARAMS_LIST,
                  XL_OP_GNB_STATS, XL_OP_HEAD_BWD, XL_OP_S2_DGRAD, XL_OP_WGRAD, XL_OP_WINO_DY, XL_OP_WINO_IN,
                  XL_OP_WINO_OUT, XL_OP_WINO_WFINAL, XlOp, act_ptr)


def _key(act):
    return (act[0].data_ptr(), act[5], act[3])          # (storage, channel offset, channels)


class _BackwardState:
    """What one backward lowering carries from tape entry to tape entry."""

    def __init__(self, plan):
        self.plan = plan
        self.ops = []
        self.grads = {}           # activation key -> (gradient tensor, ld, channel offset); layout like the activation
        self.graw = {}            # conv-output key -> dense gradient tensor
        self.gamax = {}           # conv-output key -> byte address of the slot holding max |its gradient|
        self.amax_n = 0           # slots of plan.bwd_amax handed out
        self.scratch_f = 0        # fp32 scratch (wgrad split-K partials, head / conv1 partials)
        self.scratch_d = 0        # fp64 scratch (GroupNorm backward sums)
        self.patch_f, self.patch_d = [], []      # ops whose stats2 is the fp32 / fp64 scratch, patched in once its size is known
        self.patch_bco = []       # (op, offset): conv1's folded apply reads the coefficients its GNB_FINAL left in the fp64 scratch
        self.c1_fold = {}         # conv1-output key -> what conv1's weight gradient needs to apply the GroupNorm backward on load
        self.cursor = 0           # floats of plan.grad_flat handed out
        self.producers = {_key(e["raw"]): e for e in plan.tape if e["kind"] in ("conv", "conv1")}
        # d gamma / d beta / d bias of ALL layers come from one launch at the end of the pass (XL_OP_GNB_PARAMS_LIST): a layer's
        # per-(image, channel) sums then live in a buffer of their own (XL_GNB_PARAMS_PER_LAYER=1: one launch each)
        self.params_list = None if plan.sw.GNB_PARAMS_PER_LAYER else []

    def emit(self, op, scratch_f=None, scratch_d=None):
        """Append `op`; scratch_f / scratch_d: it uses that many elements of the shared fp32 / fp64 scratch as stats2."""
        if scratch_f is not None:
            self.scratch_f = max(self.scratch_f, scratch_f)
            self.patch_f.append(len(self.ops))
        if scratch_d is not None:
            self.scratch_d = max(self.scratch_d, scratch_d)
            self.patch_d.append(len(self.ops))
        self.ops.append(op)

    def new_slot(self):
        assert self.amax_n < 1024
        self.amax_n += 1
        return self.plan.bwd_amax.data_ptr() + 4 * (self.amax_n - 1)

    def pgrad(self, param):
        """The parameter's gradient: the next (16-byte aligned) slice of the plan's flat buffer."""
        plan, n = self.plan, param.numel()
        t = plan.grad_flat[self.cursor:self.cursor + n]
        plan.param_grads.append((param, t))
        plan.grad_slices.append((param, self.cursor, n))
        self.cursor += (n + 3) // 4 * 4
        assert self.cursor <= plan.grad_flat.numel()
        return t

    def find_grad(self, act):
        """Gradient of an activation: its own entry, or a channel slice of a wider tensor's gradient
        (the three encoder outputs are slices of the MLR concat buffer)."""
        k = _key(act)
        if k in self.grads:
            return self.grads[k]
        ptr, off, C = k
        for (p2, o2, c2), (gt, gld, goff) in self.grads.items():
            if p2 == ptr and o2 <= off and off + C <= o2 + c2:
                return (gt, gld, goff + off - o2)
        return None


class _BackwardLowering:
    _key = staticmethod(_key)

    def _lower_backward(self):
        dev = self.device
        # round 5: backward GEMMs as fp16 pairs (XL_TRAIN_PAIR_BWD=0: six-pass bf16).  A gradient has no static bound: every
        # GroupNorm-backward apply pass records max |dx| (a float's bits, atomicMax) in a slot of its own, and so does the dY
        # transform of a Winograd weight gradient; the GEMMs that read those tensors derive their power-of-two scale from the
        # slot.  The slots are zeroed by the first op of the list.
        self.pair_bwd = self.pair_ok() and self.sw.TRAIN_PAIR_BWD
        self.bwd_amax = torch.zeros(1024, dtype=torch.int32, device=dev)
        st = _BackwardState(self)
        if self.pair_bwd:
            st.emit(XlOp(type=XL_OP_FILL0, Cin=4 * 1024, out=self.bwd_amax.data_ptr()))
        # every parameter gradient is a slice of ONE flat buffer (16-byte aligned slices): a backward pass hands its result
        # out with one device-to-device copy of that buffer instead of one clone per parameter (run_backward)
        total = sum((p.numel() + 3) // 4 * 4 for p in self.net.parameters() if p.requires_grad)
        self.grad_flat = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        lower = {"head": self._bwd_head, "duc_head": self._bwd_head, "gn": self._bwd_gn, "conv": self._bwd_conv,
                 "conv1": self._bwd_conv1}
        for e in reversed(self.tape):
            if not e.get("frozen"):           # frozen encoder (the reference's networks/networks.py:424-428): nothing to do
                lower[e["kind"]](st, e)
        if st.params_list:
            self.gnb_params_table = torch.from_numpy(
                np.array(st.params_list, dtype=GNB_PARAMS_ITEM_DTYPE).view(np.uint8).copy()).to(dev)
            st.emit(XlOp(type=XL_OP_GNB_PARAMS_LIST, Cin=len(st.params_list), Cout=max(i[6] for i in st.params_list),
                         in_=self.gnb_params_table.data_ptr()))
        self.bwd_scratch_f = torch.empty(max(st.scratch_f, 1), dtype=torch.float32, device=dev)
        self.bwd_scratch_d = torch.empty(max(st.scratch_d, 1), dtype=torch.float64, device=dev)
        self.bwd_array = (XlOp * len(st.ops))(*st.ops)
        for i in st.patch_f:
            self.bwd_array[i].stats2 = self.bwd_scratch_f.data_ptr()
        for i in st.patch_d:
            self.bwd_array[i].stats2 = self.bwd_scratch_d.data_ptr()
        for i, off_d in st.patch_bco:
            self.bwd_array[i].bias = self.bwd_scratch_d.data_ptr() + 8 * off_d

    def _bwd_head(self, st, e):
        """HEAD_BWD / DUC_HEAD_BWD: d(head input), d fc3.weight, d fc3.bias; dout and the forward output are patched in per call."""
        t, H, W, C, ld, off = e["x"]
        B, nc, duc = self.B, e["cout"], e["kind"] == "duc_head"
        gin = self.alloc(B * H * W * C)
        op = XlOp(type=XL_OP_DUC_HEAD_BWD if duc else XL_OP_HEAD_BWD, B=B, Hi=H, Wi=W, Cin=C, Cout=nc, n_task=e["n_task"],
                  ld_in=ld, ld_out=C, clamp_lo=-16.10, clamp_hi=13.82,
                  in_=act_ptr(e["x"]), w=e["w3"].data_ptr(), out=gin.data_ptr(),
                  out2=st.pgrad(e["fc3"].weight).data_ptr(), stats=st.pgrad(e["fc3"].bias).data_ptr())
        if duc:
            op.Ho, op.Wo = self.H, self.W
            blocks = max(1, min(1024, (B * self.H * self.W + 255) // 256))
            # (+ d(interpolated activation) [B][nc][H][W] when the bilinear trim is active)
            scratch = (blocks + 1) * (nc * nc + nc) + B * nc * self.H * self.W
        else:
            waves = 4 * max(1, min(256, (B * H * W + 63) // 64))
            scratch = waves * nc * (C + 1)
        self.head_bwd_index = len(st.ops)
        st.emit(op, scratch_f=scratch)
        st.grads[_key(e["x"])] = (gin, C, 0)

    def _bwd_gn(self, st, e):
        t, H, W, C, ld, off = e["raw"]
        B = self.B
        gout = st.find_grad(e["out"])
        if gout is None:
            return                                     # output unused downstream of any trainable path
        flags = e["flags"]
        prod = st.producers.get(_key(e["raw"]))
        # conv1's GroupNorm: its dx has ONE reader, conv1's weight gradient (the image needs no data gradient) - that kernel
        # applies the backward pass on load and the apply pass (2.1 GB read and written at batch 16) is not run
        fold_c1 = (prod is not None and prod["kind"] == "conv1" and e["aux"] is None and C == 32
                   and not (flags & (GN_ADD | GN_RELU_OUT)) and ld % 4 == 0 and off % 4 == 0
                   and not self.sw.NO_CONV1_WGRAD_FOLD)
        dx = None if fold_c1 else self.alloc(B * H * W * C)
        daux = None
        if e["aux"] is not None:
            daux = st.find_grad(e["aux"])
            if daux is not None:
                flags |= GN_ACC_AUX
            else:
                daux = (self.alloc(B * H * W * C), C, 0)
                st.grads[_key(e["aux"])] = daux
        G = e["norm"].num_groups
        nch2 = max(1, min(128, (H * W + 63) // 64))
        scratch_d = B * nch2 * C * 3 + B * C * 6 + (B * C * 3 + 1) // 2
        sums = None
        if st.params_list is not None:
            sums = torch.empty(B * C * 6, dtype=torch.float64, device=self.device)
            self.keep.append(sums)
        for typ in (XL_OP_GNB_STATS, XL_OP_GNB_FINAL, XL_OP_GNB_APPLY, XL_OP_GNB_PARAMS):
            if typ == XL_OP_GNB_APPLY and fold_c1:
                continue
            op = XlOp(type=typ, B=B, Hi=H, Wi=W, Cin=C, groups=G, nchunks2=nch2, flags=flags, eps=e["norm"].eps,
                      ld_in=ld, ld_aux=gout[1], ld_out=e["out"][4], in_=act_ptr(e["raw"]),
                      w=e["gamma"].data_ptr(), bias=e["beta"].data_ptr(), stats=e["table"].data_ptr(),
                      aux=gout[0].data_ptr() + 4 * gout[2], aux2=act_ptr(e["out"]))
            if typ == XL_OP_GNB_APPLY:
                op.out = dx.data_ptr()
                if self.pair_bwd and prod is not None:
                    st.gamax[_key(e["raw"])] = op.scale = st.new_slot()
                if daux is not None:
                    op.out2 = daux[0].data_ptr() + 4 * daux[2]
                    op.Cout = daux[1]                  # pixel stride of the d(residual) tensor
            elif typ == XL_OP_GNB_FINAL and sums is not None:
                op.scale = sums.data_ptr()
            elif typ == XL_OP_GNB_PARAMS:
                op.out = st.pgrad(e["norm"].weight).data_ptr()
                op.out2 = st.pgrad(e["norm"].bias).data_ptr()
                if prod is not None:
                    op.aux2 = st.pgrad(prod["conv"].bias).data_ptr()
                else:
                    op.flags = flags | GN_NO_CONV_BIAS
                if sums is not None:
                    st.params_list.append((sums.data_ptr(), e["gamma"].data_ptr(), op.out, op.out2,
                                           op.aux2 if prod is not None else 0, B, C, G, H * W))
                    continue
            st.emit(op, scratch_d=scratch_d)
        if fold_c1:
            # (the gradient w.r.t. the GroupNorm output stays alive until conv1's weight gradient has read it)
            st.c1_fold[_key(e["raw"])] = dict(dout=gout, x=(t, ld, off), fco=e["table"], flags=flags,
                                              bco_off=B * nch2 * C * 3 + B * C * 6,
                                              release=st.grads.pop(_key(e["out"]), (None,))[0])
            st.graw[_key(e["raw"])] = gout[0]
            return
        if _key(e["out"]) in st.grads:                  # dense, fully consumed: recycle (slices of the
            self.release_grad(st.grads.pop(_key(e["out"]))[0])   # concat gradient stay until the end)
        if prod is not None:
            st.graw[_key(e["raw"])] = dx
        else:
            # GroupNorm applied directly to an activation (mlr_norm on the concat buffer): dx is a gradient of that activation
            assert st.find_grad(e["raw"]) is None
            st.grads[_key(e["raw"])] = (dx, C, 0)

    def _bwd_conv(self, st, e):
        conv = e["conv"]
        t, H, W, C, ld, off = e["x"]
        Cout = e["raw"][3]
        dy = st.graw.pop(_key(e["raw"]), None)
        if dy is None:
            return
        dy_amax = st.gamax.pop(_key(e["raw"]), None)
        wm = 0
        if conv.kernel_size[0] == 3 and conv.stride[0] == 1 and self.wino_wgrad_layer_ok(H, W, C, Cout):
            # a V kept by the forward pass fixes the tile size; otherwise the cheapest form for this map
            # (a deferred GroupNorm - xnorm - was accepted by wino_wgrad_ok() for the FORWARD tile size: keep it, V kept or not)
            wm = e.get("wm", 0) if (e.get("v") is not None or e.get("xnorm") is not None) else self.wino_pick(H, W, max(C, Cout))
        if wm in (4, 6) and self.B * -(-H // wm) * -(-W // wm) >= 64:
            self._bwd_wgrad_wino(st, e, dy, wm)
        else:
            self._bwd_wgrad_direct(st, e, dy, dy_amax)
        self._bwd_dgrad(st, e, dy, dy_amax)
        self.release_grad(dy)

    def _bwd_wgrad_wino(self, st, e, dy, wm):
        """Weight gradient through F(m x m,3x3): V = B^T x B, dM = A dY A^T, (m+2)^2 GEMMs over the tiles, dg = G^T dU G."""
        conv, B = e["conv"], self.B
        t, H, W, C, ld, off = e["x"]
        Cout = e["raw"][3]
        bo, bc = 128, (128 if C % 128 == 0 else 64)
        Th, Tw = -(-H // wm), -(-W // wm)
        T, nf = B * Th * Tw, (wm + 2) ** 2                    # tiles = K dimension of the GEMMs
        Vb = e.get("v")
        if Vb is None:
            Vb = self.alloc(nf * T * C)
            wi = XlOp(type=XL_OP_WINO_IN, ksize=wm, B=B, Hi=H, Wi=W, Cin=C, Ho=Th, Wo=Tw, ld_in=ld,
                      in_=act_ptr(e["x"]), out=Vb.data_ptr())
            if e.get("xnorm") is not None:                # x is a raw conv output whose GroupNorm was left to its consumers
                wi.aux2, wi.flags = e["xnorm"].aux2, e["xnorm"].flags & GN_RELU_IN
            st.emit(wi)
        dMb = self.alloc(nf * T * Cout)
        wd = XlOp(type=XL_OP_WINO_DY, ksize=wm, B=B, Hi=H, Wi=W, Cin=Cout, Ho=Th, Wo=Tw, ld_in=Cout,
                  in_=dy.data_ptr(), out=dMb.data_ptr())
        wg_pair = self.pair_bwd and wm == 6 and self.wgrad_split_ok(C, Cout)
        if wg_pair:
            wd.scale = st.new_slot()                      # max |dM|: the scale of the weight-gradient GEMMs' dY operand
        st.emit(wd)
        dU = self.alloc(nf * Cout * C)
        wg = XlOp(type=XL_OP_WGRAD, B=1, Hi=T, Wi=1, Cin=C, Ho=T, Wo=1, Cout=Cout, ksize=1, stride=1, ld_in=C, ld_aux=Cout,
                  groups=nf, in_=Vb.data_ptr(), aux=dMb.data_ptr(), out=dU.data_ptr())
        if self.wgrad_split_ok(C, Cout):
            # on the split pipe (csrc/xl_wgrad_split.hip): 256 x 256 tiles, one workgroup per CU
            wg.flags = CONV_SPLIT_BF16
            splits = self.wgrad_splits(nf * (Cout // 256) * (C // 256), T)
            if wg_pair:                                   # csrc/xl_wgrad_pair.hip: V at the plan's scale, dM at its own
                wg.flags |= CONV_PAIR_F16
                wg.scale, wg.out2 = self.pair_scales.data_ptr() + 8, wd.scale
        else:
            splits = self.split_k(nf * (Cout // bo) * (C // bc), T, bo, bc, resident=512, max_splits=32)
        wg.nchunks2 = splits
        st.emit(wg, scratch_f=nf * splits * Cout * C)
        st.emit(XlOp(type=XL_OP_WINO_WFINAL, ksize=wm, Cin=C, Cout=Cout, in_=dU.data_ptr(), out=st.pgrad(conv.weight).data_ptr()))
        self.release_grad(Vb); self.release_grad(dMb); self.release_grad(dU)   # a kept V is dead from here on

    def _bwd_wgrad_direct(self, st, e, dy, dy_amax):
        conv, B = e["conv"], self.B
        t, H, W, C, ld, off = e["x"]
        rt, Ho, Wo, Cout, rld, roff = e["raw"]
        k, s = conv.kernel_size[0], conv.stride[0]
        bo = 128 if Cout % 128 == 0 else 64
        bc = 128 if C % 128 == 0 else (64 if C % 64 == 0 else 32)
        M = B * Ho * Wo
        op = XlOp(type=XL_OP_WGRAD, B=B, Hi=H, Wi=W, Cin=C, Ho=Ho, Wo=Wo, Cout=Cout, ksize=k, stride=s, ld_in=ld, ld_aux=Cout,
                  in_=act_ptr(e["x"]), aux=dy.data_ptr())
        xnorm = e.get("xnorm")
        if k == 1 and s == 1 and self.wgrad_split_ok(C, Cout) and ld % 4 == 0 and off % 4 == 0:
            op.flags = CONV_SPLIT_BF16
            splits = self.wgrad_splits((Cout // 256) * (C // 256), M)
            if self.pair_bwd and dy_amax is not None:
                op.flags |= CONV_PAIR_F16
                op.scale, op.out2 = self.pair_scales.data_ptr(), dy_amax
            if xnorm is not None:                         # x is a raw conv output: normalise on load
                op.flags |= CONV_NORM_IN | (CONV_NORM_RELU if xnorm.flags & GN_RELU_IN else 0)
                op.aux2 = xnorm.aux2
        else:
            assert xnorm is None, "a deferred GroupNorm reached a weight-gradient form that cannot apply it"
            # (round 4: resident workgroups by the tile form's LDS - 2 stages x 32 pixels x (bo + bc) floats: the 64 x 32 form of
            #  conv2's weight gradient, 9 tiles, fits six per CU, and 56 splits = 504 two-wave workgroups had left the chip at one
            #  wave per SIMD: 0.99 -> 0.54 ms; 128 x 64 fits three)
            per_cu = 2 if self.sw.WGRAD_SMALL_SPLITS_OLD else max(2, min(6, (160 * 1024) // (2 * 32 * (bo + bc) * 4)))
            splits = self.split_k(k * k * (Cout // bo) * (C // bc), M, bo, bc, resident=256 * per_cu, max_splits=32 * per_cu)
        op.nchunks2 = splits
        op.out = st.pgrad(conv.weight).data_ptr()
        st.emit(op, scratch_f=splits * k * k * Cout * C)

    def _bwd_dgrad(self, st, e, dy, dy_amax):
        """Data gradient into the gradient of x (second producers accumulate)."""
        conv, B = e["conv"], self.B
        t, H, W, C, ld, off = e["x"]
        rt, Ho, Wo, Cout, rld, roff = e["raw"]
        k, s = conv.kernel_size[0], conv.stride[0]
        gx = st.find_grad(e["x"])
        acc = CONV_ACCUMULATE if gx is not None else 0
        if gx is None:
            gx = (self.alloc(B * H * W * C), C, 0)
            st.grads[_key(e["x"])] = gx
        gx_ptr = gx[0].data_ptr() + 4 * gx[2]
        m = self.wino_dgrad_m(conv, H, W, C)
        if m:
            # dX = conv3x3(dY, flipped kernel, channels swapped) as F(m x m,3x3): 4x / 5x fewer multiplies
            Th, Tw = -(-H // m), -(-W // m)
            T, nf = B * Th * Tw, (m + 2) ** 2
            Vb = self.alloc(nf * T * Cout)
            st.emit(XlOp(type=XL_OP_WINO_IN, ksize=m, B=B, Hi=H, Wi=W, Cin=Cout, Ho=Th, Wo=Tw, ld_in=Cout,
                         in_=dy.data_ptr(), out=Vb.data_ptr()))
            Mb = self.alloc(nf * T * C)
            gm = XlOp(type=XL_OP_CONV, B=B, Hi=Th, Wi=Tw, Cin=Cout, Ho=Th, Wo=Tw, Cout=C, ksize=1, stride=1, ld_in=Cout, ld_out=C,
                      nchunks2=nf, in_=Vb.data_ptr(), out=Mb.data_ptr())
            tile_major = 0
            if self.wino_gemm_form(Cout, C, m, T)[2]:       # on the split pipe, V(dY) split inside the GEMM kernel
                tile_major = CONV_M_TILE_MAJOR if (m == 6 and self.sw.WINO_M_TILE_MAJOR) else 0
                gm.flags = CONV_SPLIT_BF16 | CONV_SPLIT_IL | CONV_SPLIT_ACT | tile_major
                if self.pair_bwd and dy_amax is not None and not tile_major:
                    # V(dY) stays fp32; the pairs are formed in the GEMM at the scale of max |dY| / 256 (|B^T d B| <= 225 max|d|)
                    gm.flags |= CONV_PAIR_F16 | CONV_PAIR_AMAX
                    gm.w = self.pack_conv_wino_pair(conv, m, dgrad=True).data_ptr()
                    gm.scale = dy_amax
                else:
                    gm.w = self.pack_conv_wino_split(conv, m, True, dgrad=True).data_ptr()
            else:
                gm.w = self.pack_conv_wino(conv, m, dgrad=True).data_ptr()
                if -(-T // 128) * (C // 128) * nf <= 256:
                    gm.reserved_i = 64
            st.emit(gm)
            tpb = self.wino_out_tpb(m, Th * Tw, C)
            st.emit(XlOp(type=XL_OP_WINO_OUT, ksize=m, B=B, Hi=H, Wi=W, Cin=C, ld_out=gx[1], groups=1,
                         nchunks=-(-(Th * Tw) // tpb), reserved_i=tpb, flags=acc | tile_major, in_=Mb.data_ptr(), out=gx_ptr))
            self.release_grad(Vb); self.release_grad(Mb)
            return
        op = XlOp(type=XL_OP_CONV, flags=CONV_DGRAD | acc, B=B, Hi=Ho, Wi=Wo, Cin=Cout, Ho=H, Wo=W, Cout=C,
                  ksize=k, stride=s, ld_in=Cout, ld_out=gx[1], in_=dy.data_ptr(), out=gx_ptr)
        aligned = gx[1] % 4 == 0 and gx[2] % 4 == 0 and self.split_train_ok() and self.sw.split_on
        if k == 3 and s == 2 and (Cout, C) in ((64, 32), (128, 64)) and not acc and aligned and not self.sw.NO_S2_DGRAD:
            # round 4: the stem's data gradients on the split pipe, one launch over tiles of the result instead of four
            # parity-class launches of the fp32 implicit GEMM (csrc/xl_stem_dgrad.hip)
            op.type, op.flags = XL_OP_S2_DGRAD, 0
            op.w = self.pack_s2_dgrad_fragments(conv).data_ptr()
            queue = torch.zeros(4, dtype=torch.int32, device=self.device)
            self.keep.append(queue)
            op.stats = queue.data_ptr()
        elif (k == 1 and s == 1 and Cout % 32 == 0 and C % 256 == 0 and C <= 1024 and H * W >= 256 and aligned
              and not self.sw.NO_SPLIT_1X1):
            # dX = dY W on the split pipe: a plain 1x1 "convolution" of dY with the transposed weight matrix, split
            # once per weight version; a second producer of the gradient accumulates in the epilogue
            op.flags = CONV_SPLIT_BF16 | CONV_SPLIT_IL | acc
            if self.pair_bwd and dy_amax is not None:
                op.flags |= CONV_PAIR_F16 | CONV_PAIR_AMAX
                op.w = self.pack_conv_1x1_pair(conv, transposed=True).data_ptr()
                op.scale = dy_amax
            else:
                op.w = self.pack_conv_1x1_split(conv, transposed=True).data_ptr()
            op.reserved_i = 256
        else:
            op.w = self.pack_conv(conv, dgrad=True).data_ptr()
        st.emit(op)          # 32 result channels (conv2): the kernel masks the padded half of its 64-wide tile

    def _bwd_conv1(self, st, e):
        conv = e["conv"]
        rt, H, W, Cout, rld, roff = e["raw"]
        dy = st.graw.pop(_key(e["raw"]), None)
        if dy is None:
            return
        op = XlOp(type=XL_OP_CONV1_WGRAD, B=self.B, Hi=H, Wi=W, Cin=conv.in_channels, Cout=Cout, ld_aux=Cout, aux=dy.data_ptr(),
                  reserved_i=8)                               # image rows per workgroup
        fold = st.c1_fold.pop(_key(e["raw"]), None)
        if fold is not None:                                # the GroupNorm-backward apply pass on load (see _bwd_gn)
            gt, gld, goff = fold["dout"]
            xt, xld, xoff = fold["x"]
            op.aux, op.ld_aux = gt.data_ptr() + 4 * goff, gld
            op.aux2, op.ld_in = xt.data_ptr() + 4 * xoff, xld
            op.w, op.flags = fold["fco"].data_ptr(), fold["flags"]
            st.patch_bco.append((len(st.ops), fold["bco_off"]))
        op.out = st.pgrad(conv.weight).data_ptr()
        # the bias gradient of conv1 comes from the GroupNorm backward sums (fp64 closed form); the sum this
        # kernel also produces goes to a scratch vector
        self.conv1_db_unused = torch.empty(Cout, dtype=torch.float32, device=self.device)
        op.out2 = self.conv1_db_unused.data_ptr()
        self.conv1_wgrad_indices.append(len(st.ops))
        st.emit(op, scratch_f=self.B * ((H + 7) // 8) * 28 * Cout)
        if fold is None:
            self.release_grad(dy)
        elif fold["release"] is not None:
            self.release_grad(fold["release"])
