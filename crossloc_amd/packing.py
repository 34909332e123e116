"""Weight operands of a plan: packing of the convolution weights into the layouts the kernels read (direct, Winograd,
split-bf16 planes, fp16 pairs, MFMA fragments of the stem), the static activation scales of the pair GEMMs, and their
refresh after an in-place parameter update.  Mixed into `networks._Plan`."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import switches
from .ops import (PAIR_ITEM_DTYPE, XL_OP_GN_APPLY, XL_OP_GN_FINAL, _bind, _check)


class _Packing:
    # -- weights
    # Winograd F(2x2,3x3) weight transform U = G g G^T, G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]] (Lavin & Gray 2016)
    _WINO_G = {2: ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0)),
               # F(4x4,3x3), interpolation points 0, +-1, +-2, inf
               4: ((1 / 4, 0.0, 0.0), (-1 / 6, -1 / 6, -1 / 6), (-1 / 6, 1 / 6, -1 / 6), (1 / 24, 1 / 12, 1 / 6),
                   (1 / 24, -1 / 12, 1 / 6), (0.0, 0.0, 1.0)),
               # F(6x6,3x3), interpolation points 0, +-1, +-2, +-1/2, inf (the scaling of Lavin's wincnn set)
               6: ((1.0, 0.0, 0.0), (-2 / 9, -2 / 9, -2 / 9), (-2 / 9, 2 / 9, -2 / 9), (1 / 90, 1 / 45, 2 / 45),
                   (1 / 90, -1 / 45, 2 / 45), (1 / 45, 1 / 90, 1 / 180), (1 / 45, -1 / 90, 1 / 180), (0.0, 0.0, 1.0))}

    def pack_conv_wino(self, conv, m, dgrad=False):
        """[(m+2)^2][Cout][Cin] transformed weights of a 3x3 convolution: one plain [Cout][Cin] GEMM operand per
        frequency of F(m x m, 3x3).  dgrad: the data gradient is the convolution with the flipped kernel and the
        channel roles swapped, so its operands are [(m+2)^2][Cin][Cout]."""
        kind = "wino%d%s" % (m, "d" if dgrad else "")
        return self._packed(conv, (id(conv.weight), kind), kind, (m + 2) ** 2 * conv.out_channels * conv.in_channels)

    @staticmethod
    def split_bf16(x):
        """fp32 tensor -> [3, ...] bf16 planes with x = p0 + p1 + p2 exactly (8 + 8 + 8 mantissa bits), as int16 storage."""
        p0 = x.to(torch.bfloat16)
        r1 = x - p0.to(torch.float32)
        p1 = r1.to(torch.bfloat16)
        p2 = (r1 - p1.to(torch.float32)).to(torch.bfloat16)
        return torch.stack([p0, p1, p2]).contiguous().view(torch.int16)

    @staticmethod
    def split_bf16_interleaved(x, C):
        """fp32 tensor whose last dimension runs over C channels -> the interleaved-plane operand layout of the 256 x 256
        split GEMM, [..., C/16, 3, 16] bf16 (as int16 storage): the three planes of a 16-channel chunk next to each other."""
        planes = _Packing.split_bf16(x.reshape(-1, C // 16, 16)).view(3, -1, C // 16, 16)
        return planes.permute(1, 2, 0, 3).contiguous()

    def pack_conv_wino_split(self, conv, m, interleaved=False, dgrad=False):
        """The transformed weights of pack_conv_wino as three bf16 planes (operands of csrc/xl_gemm_split.hip): separate
        planes, or - `interleaved` - [(m+2)^2][Cout][Cin/16][3][16] for the 256 x 256 kernel."""
        key = (id(conv.weight), "wino%d%s_split%s" % (m, "d" if dgrad else "", "_il" if interleaved else ""))
        if key not in self.packed_split:
            src = self.dev_weight(conv)
            planes = torch.empty(3 * (m + 2) ** 2 * src.shape[0] * src.shape[1], dtype=torch.int16, device=self.device)
            self.packed_split[key] = (planes, src, m, interleaved, dgrad)
            self._pack_wino_split(*self.packed_split[key])
        return self.packed_split[key][0]

    def _pack_wino_split(self, planes, src, m, interleaved, dgrad=False):
        """U = G g G^T (float64 inside) and its exact three-term bf16 split in one HIP launch (csrc/xl_pack.hip); dgrad: the
        data-gradient operand [(m+2)^2][Cin][Cout] (flipped kernel, channel roles swapped)."""
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(_bind().xl_cnn_pack_wino_weight(src.data_ptr(), planes.data_ptr(), src.shape[0], src.shape[1], m,
                                               1 if dgrad else 0, 2 if interleaved else 1, stream))

    def _split_weight(self, planes, src, transposed=False):
        """fp32 [rows][K] (1x1; `transposed`: rows and K swapped) or OIHW 3x3 (K tap-major) -> interleaved bf16 planes, one
        HIP launch."""
        taps = 9 if (src.dim() == 4 and src.shape[2] == 3) else 1
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if transposed:
            _check(_bind().xl_cnn_split_weight(src.data_ptr(), planes.data_ptr(), src.shape[1], src.shape[0], 0, stream))
        else:
            _check(_bind().xl_cnn_split_weight(src.data_ptr(), planes.data_ptr(), src.shape[0], src.shape[1] * taps, taps, stream))

    def _gn_layers(self):
        """(gamma, beta, C, sqrt(N)) of every GroupNorm of the network: N = the elements of a group, from the op that applies
        the layer in this plan, or - layers the plan does not run - from the image size (no map is larger)."""
        seen = {}
        for op in self.ops:
            if op.type in (XL_OP_GN_FINAL, XL_OP_GN_APPLY) and op.w and op.bias and op.groups > 0:
                n = (op.Cin // op.groups) * op.Hi * op.Wi
                seen[op.w] = max(seen.get(op.w, 0), n)
        out = []
        for mod in self.net.modules():
            if not isinstance(mod, nn.GroupNorm):
                continue
            if mod.weight is None:
                # affine=False (no reference network has one): gamma = 1, beta = 0 in the bound - constants of the plan
                if mod.num_channels not in self._unit_gn:
                    self._unit_gn[mod.num_channels] = (torch.ones(mod.num_channels, dtype=torch.float32, device=self.device),
                                                       torch.zeros(mod.num_channels, dtype=torch.float32, device=self.device))
                g, b = self._unit_gn[mod.num_channels]
                n = (mod.num_channels // mod.num_groups) * self.H * self.W
            else:
                # (not self.dev(): this runs with every weight refresh and must not grow the plan's keep list - the tensors alias the
                #  live parameters and are held by the caller's table)
                g = mod.weight.detach().to(device=self.device, dtype=torch.float32).contiguous()
                b = mod.bias.detach().to(device=self.device, dtype=torch.float32).contiguous()
                n = seen.get(g.data_ptr(), (mod.num_channels // mod.num_groups) * self.H * self.W)
            out.append((g, b, mod.num_channels, float(n) ** 0.5))
        return out

    def _update_pair_scales(self):
        """s = the largest power of two with s * sum over the GroupNorm layers of (sqrt(N) max|gamma| + max|beta|) <= 2^14:
        |gn(x)| <= sqrt(N - 1) |gamma| + |beta|, an activation is a GroupNorm output plus residuals that are activations
        themselves (the sum over ALL layers bounds any chain), and |B^T d B| <= 225 max|d| for F(6x6,3x3).  One tiny launch
        reading the live parameters - no host synchronisation, so a training loop can call it every step."""
        if not self.pair_ok():
            return
        # (the table holds raw device pointers of gamma / beta: rebuilt whenever a parameter's storage moved - net.to(),
        #  load_state_dict(assign=True) -, as _repack_pairs re-validates its own tables)
        layers = self._gn_layers()
        sig = tuple((g.data_ptr(), b.data_ptr()) for g, b, _, _ in layers)
        if self._pair_gn_sig != sig:
            self._pair_gn_keep = [(g, b) for g, b, _, _ in layers]
            self._pair_gn_sig = sig
            n = len(layers)
            self._pair_gn = ((ctypes.c_void_p * n)(*[g.data_ptr() for g, _, _, _ in layers]),
                             (ctypes.c_void_p * n)(*[b.data_ptr() for _, b, _, _ in layers]),
                             (ctypes.c_int * n)(*[c for _, _, c, _ in layers]),
                             (ctypes.c_float * n)(*[r for _, _, _, r in layers]), n)
        g, b, c, r, n = self._pair_gn
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _check(_bind().xl_cnn_pair_scales(g, b, c, r, n, self.pair_scales.data_ptr(), stream))

    def _pair_operand(self, conv, kind, floats, m=0, mode=""):
        """The cached fp16-pair operand `kind` of a convolution's weight, packed on first use: 2 int16 per weight + `floats`
        fp32 words (scratch maxima, inverse scales) behind them."""
        key = (id(conv.weight), kind)
        if key not in self.packed_pair:
            src = self.dev_weight(conv)
            nf = (m + 2) ** 2 if m else 1
            planes = torch.empty(2 * nf * src.numel() // (9 if m else 1) + 2 * floats, dtype=torch.int16, device=self.device)
            self.packed_pair[key] = (planes, src, m, mode)
            self._pack_pair(*self.packed_pair[key])
        return self.packed_pair[key][0]

    def pack_conv_wino_pair(self, conv, m, dgrad=False):
        """The transformed weights of pack_conv_wino as fp16 pairs {hi, lo} [(m+2)^2][Cout][Cin/16][2][16], each frequency scaled by its
        own power of two, + 2 (m+2)^2 floats (scratch, inverse scales).  dgrad: the data-gradient operand [(m+2)^2][Cin][Cout/16]..."""
        d = "d" if dgrad else ""
        return self._pair_operand(conv, "wino%d%s_pair" % (m, d), 2 * (m + 2) ** 2, m, d)

    def pack_conv_1x1_pair(self, conv, transposed=False):
        """[Cout][Cin/16][2][16] fp16 pairs {hi, lo} of a 1x1 convolution's weight (one power-of-two scale) + 2 floats;
        `transposed`: [Cin][Cout/16][2][16], the operand of its data gradient."""
        return self._pair_operand(conv, "1x1_pair" + ("_t" if transposed else ""), 2, 0, "t" if transposed else "")

    def pack_conv_stem_pair(self, conv):
        """[Cout][9 Cin / 16][2][16] fp16 pairs {hi, lo} of a 3x3 convolution's weight, K ordered tap-major, + 2 floats."""
        return self._pair_operand(conv, "stem_pair", 2)

    def _pack_pair(self, planes, src, m, mode=""):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if m:
            _check(_bind().xl_cnn_pack_wino_weight_pair(src.data_ptr(), planes.data_ptr(), src.shape[0], src.shape[1], m,
                                                        1 if mode == "d" else 0, stream))
        elif mode == "t":                             # [Cin][Cout]: rows and K swapped
            _check(_bind().xl_cnn_pair_weight(src.data_ptr(), planes.data_ptr(), src.shape[1], src.shape[0], 0, stream))
        elif src.dim() == 4 and src.shape[2] == 3:
            _check(_bind().xl_cnn_pair_weight(src.data_ptr(), planes.data_ptr(), src.shape[0], src.shape[1] * 9, 9, stream))
        else:
            _check(_bind().xl_cnn_pair_weight(src.data_ptr(), planes.data_ptr(), src.shape[0], src.shape[1], 1, stream))

    @staticmethod
    def _pair_item(planes, src, m, mode=""):
        """(list key, rows, K, kind) of a packed_pair entry for xl_cnn_repack_pairs - the arguments _pack_pair passes per matrix."""
        if m:
            return m, src.shape[0], src.shape[1], 1 if mode == "d" else 0
        if mode == "t":
            return 0, src.shape[1], src.shape[0], 0
        if src.dim() == 4 and src.shape[2] == 3:
            return 0, src.shape[0], src.shape[1] * 9, 9
        return 0, src.shape[0], src.shape[1], 1

    def _repack_pairs(self):
        """Every fp16-pair operand again (refresh_weights) in three launches per list - the F(6x6,3x3) layers, the F(4x4,3x3) ones,
        the plain matrices - instead of a memset and two launches per matrix (xl_cnn_repack_pairs; 24 + 23 matrices per step of
        the batch-16 training plan).  The device tables hold pointers: they are rebuilt when an entry or an address changed."""
        if not self.packed_pair:
            return
        if switches.live("XL_NO_BATCHED_REPACK"):
            for entry in self.packed_pair.values():
                self._pack_pair(*entry)
            return
        entries = list(self.packed_pair.values())
        sig = tuple((e[0].data_ptr(), e[1].data_ptr()) for e in entries)
        if self._pair_tables_sig != sig:
            lists = {}
            for planes, src, m, mode in entries:
                key, rows, K, kind = self._pair_item(planes, src, m, mode)
                lists.setdefault(key, []).append((src.data_ptr(), planes.data_ptr(), rows, K, kind, 0))
            dt = PAIR_ITEM_DTYPE
            self._pair_tables = []
            for key, items in sorted(lists.items()):
                table = torch.from_numpy(np.array(items, dtype=dt).view(np.uint8).copy()).to(self.device)
                self._pair_tables.append((key, len(items), max(i[2] * i[3] for i in items), table))
            self._pair_tables_sig = sig
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for key, n, biggest, table in self._pair_tables:
            _check(_bind().xl_cnn_repack_pairs(table.data_ptr(), n, key, biggest, stream))

    def pack_conv(self, conv, dgrad=False):
        kind = "conv1" if (conv.in_channels in (1, 3) and conv.kernel_size[0] == 3) else ("dgrad" if dgrad else "fwd")
        return self._packed(conv, (id(conv.weight), dgrad), kind, conv.weight.numel())

    def _packed(self, conv, key, kind, numel):
        """The cached fp32 operand `kind` of a convolution's weight (see _pack), packed on first use."""
        if key not in self.packed:
            src = self.dev_weight(conv)
            dst = torch.empty(numel, dtype=torch.float32, device=self.device)
            self.packed[key] = (dst, src, kind)
            self._pack(dst, src, kind)
        return self.packed[key][0]

    def _pack(self, dst, src, kind):
        L = _bind()
        cout, cin, k, _ = src.shape
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if kind.startswith("wino"):                  # U = G g G^T in float64, rounded once: one HIP launch (csrc/xl_pack.hip)
            _check(L.xl_cnn_pack_wino_weight(src.data_ptr(), dst.data_ptr(), cout, cin, int(kind[4]),
                                             1 if kind.endswith("d") else 0, 0, stream))
        elif kind == "conv1":                     # [(ky*3+kx)*Cin + c][Cout]
            dst.view(k, k, cin, cout).copy_(src.permute(2, 3, 1, 0))
        elif kind == "dgrad":
            _check(L.xl_cnn_pack_conv_weight_dgrad(src.data_ptr(), dst.data_ptr(), cout, cin, k, stream))
        else:
            _check(L.xl_cnn_pack_conv_weight(src.data_ptr(), dst.data_ptr(), cout, cin, k, stream))

    def refresh_weights(self):
        """Parameters changed in place (optimizer step, load_state_dict): re-pack the conv operands.  Biases,
        GroupNorm affine parameters and fc3 are read through pointers to the live parameters."""
        for dst, src, kind in self.packed.values():
            self._pack(dst, src, kind)
        for entry in self.packed_split.values():
            self._pack_wino_split(*entry)
        for entry in self.packed_1x1.values():
            self._split_weight(*entry)
        self._repack_pairs()
        self._update_pair_scales()
        for key, (planes, src) in self.packed_c1.items():
            kind = key[1] if isinstance(key, tuple) else "c1"
            planes.copy_(self.conv2_pair_fragments(src) if kind == "c2pair" else      # (src: the conv module)
                         self.s2_dgrad_fragments(src) if kind == "s2dgrad" else self.conv2_fragments(src) if kind == "c2frag"
                         else self.conv1_fragments(src))

    def dev_weight(self, conv):
        """The convolution's weight as a device fp32 tensor: an alias of the live parameter whenever that is one already."""
        return conv.weight.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def dev(self, p):
        t = p.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.keep.append(t)
        return t

    def pack_conv_stem_split(self, conv):
        """[Cout][9 Cin / 16][3][16] bf16: the weight of a 3x3 convolution with K ordered tap-major (K = (3 ky + kx) Cin + c)
        as interleaved bf16 planes (_split_weight tells the two layouts apart by the weight's shape)."""
        return self.pack_conv_1x1_split(conv)

    @staticmethod
    def _stem_rows(src):
        return src.permute(0, 2, 3, 1).reshape(src.shape[0], -1) if src.dim() == 4 and src.shape[2] == 3 else src.reshape(src.shape[0], src.shape[1])

    def pack_conv_1x1_split(self, conv, transposed=False):
        """[Cout][Cin/16][3][16] bf16: the weight of a 1x1 convolution as interleaved bf16 planes; `transposed`:
        [Cin][Cout/16][3][16], the operand of its data gradient."""
        w = conv.weight
        key = (id(w), "t") if transposed else id(w)
        if key not in self.packed_1x1:
            src = self.dev_weight(conv)
            planes = torch.empty(3 * src.numel(), dtype=torch.int16, device=self.device)
            self.packed_1x1[key] = (planes, src, transposed)
            self._split_weight(planes, src, transposed)
        return self.packed_1x1[key][0]

    _conv1_fragment_index = {}                   # device -> gather indices of conv1_fragments

    @staticmethod
    def conv1_fragments(weight):
        """[3 planes][3 window rows][64 lanes][8] bf16 (int16 storage): the MFMA weight fragments of conv1_mfma_kernel.  Lane =
        32 * K-half + output channel; slot i of a lane = (dx = 2 * K-half + i // 4, c = i % 4), zero for c = 3 and dx = 3."""
        w = weight.detach().to(torch.float32)                                    # [32][3][ky][kx]
        # one gather through an index table (a training loop rebuilds the fragments after every step): slot (dy, K-half, channel,
        # i) <- w[channel][c][dy][dx], or the zero appended behind the weights
        idx = _Packing._conv1_fragment_index.get(w.device)
        if idx is None:
            host = torch.full((3, 2, 32, 8), 32 * 27, dtype=torch.int64)
            for dy in range(3):
                for kh in range(2):
                    for i in range(8):
                        dx, c = 2 * kh + i // 4, i % 4
                        if c < 3 and dx < 3:
                            host[dy, kh, :, i] = torch.arange(32) * 27 + c * 9 + dy * 3 + dx
            idx = _Packing._conv1_fragment_index[w.device] = host.reshape(-1).to(w.device)
        f = torch.cat([w.reshape(-1), w.new_zeros(1)])[idx]                      # [dy][K-half][channel][slot]
        planes = _Packing.split_bf16(f.reshape(3, 64, 8))                           # [3 planes][3 dy][64][8]
        return planes.contiguous()

    @staticmethod
    def conv2_fragments(weight):
        """[18 K-steps][3 planes][2 column blocks][64 lanes][8] bf16 (int16 storage): the MFMA weight fragments of stem12_kernel
        (csrc/xl_stem_fused.hip) for the 32 -> 64 3x3 stride-2 layer.  K = tap * 32 + channel (tap = 3 ky + kx), a K-step = 16
        channels of one tap; lane = 32 * K-half + output channel within the 32-channel block; a lane's 8 values are consecutive K."""
        w = weight.detach().to(torch.float32)                                    # [64][32][ky][kx]
        rows = w.permute(0, 2, 3, 1).reshape(64, 288)
        planes = _Packing.split_bf16(rows).view(3, 2, 32, 18, 2, 8)                 # [plane][j][fr][kk][kh][8]
        return planes.permute(3, 0, 1, 4, 2, 5).contiguous()                     # [kk][plane][j][kh][fr][8]

    @staticmethod
    def s2_dgrad_fragments(weight):
        """[9 taps][CO/16][3 planes][CI/32][64 lanes][8] bf16 (int16 storage): the MFMA weight fragments of s2_dgrad_kernel
        (csrc/xl_stem_dgrad.hip) for a stride-2 3x3 layer with weight [CO][CI][3][3]: rows = the layer's INPUT channels (the
        gradient's channels), K = its output channels; lane = 32 * K-half + row within the 32-row block."""
        w = weight.detach().to(torch.float32)
        CO, CI = w.shape[0], w.shape[1]
        wt = w.permute(2, 3, 1, 0).reshape(9, CI, CO)                            # [tap][ci][co]
        planes = _Packing.split_bf16(wt).view(3, 9, CI // 32, 32, CO // 16, 2, 8)   # [plane][tap][j][fr][c][kh][8]
        return planes.permute(1, 4, 0, 2, 5, 3, 6).contiguous()                  # [tap][c][plane][j][kh][fr][8]

    def _fragments(self, conv, key, make):
        """The cached MFMA weight fragments `make(weight)` of a stem layer; refresh_weights() rebuilds them by the key's kind."""
        if key not in self.packed_c1:
            src = self.dev_weight(conv)
            self.packed_c1[key] = (make(src), src)
        return self.packed_c1[key][0]

    def pack_s2_dgrad_fragments(self, conv):
        return self._fragments(conv, (id(conv.weight), "s2dgrad"), self.s2_dgrad_fragments)

    def pack_conv2_fragments(self, conv):
        return self._fragments(conv, (id(conv.weight), "c2frag"), self.conv2_fragments)

    def pack_conv1_split(self, conv):
        return self._fragments(conv, id(conv.weight), self.conv1_fragments)

    def conv2_pair_fragments(self, conv):
        """[18 K-steps][2 planes {hi, lo}][2 column blocks][64 lanes][8] fp16 + the inverse weight scale (one float, then padding
        to 16 bytes): the MFMA weight fragments of stem12_kernel<.., true> - the pair form of the 32 -> 64 stride-2 layer, cut
        from the operand xl_cnn_pair_weight packs for pair_conv3x3s2_kernel (same scale, same split: the fused and the
        two-kernel stem stay bitwise equal).  (int16 storage)"""
        packed = self.pack_conv_stem_pair(conv)                                  # (a refresh re-packs packed_pair first: _repack_pairs)
        n = 64 * 288
        frag = packed[:2 * n].view(2, 32, 18, 2, 2, 8).permute(2, 3, 0, 4, 1, 5).contiguous().reshape(-1)   # [kk][p][j][kh][fr][8]
        tail = torch.zeros(8, dtype=torch.int16, device=self.device)
        tail[:2] = packed[2 * n + 2:2 * n + 4]                                   # the inverse scale (behind the maxima word)
        return torch.cat([frag, tail])

    def pack_conv2_pair_fragments(self, conv):
        key = (id(conv.weight), "c2pair")
        if key not in self.packed_c1:
            self.packed_c1[key] = (self.conv2_pair_fragments(conv), conv)
        return self.packed_c1[key][0]
