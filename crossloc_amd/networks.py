"""MI355X-native `TransPoseNet` — same constructor, attributes and state_dict keys as the reference
(networks/networks.py:375-502 there) so `load_state_dict` on reference checkpoints is strict-clean
(116 tensors single-task, 270 for the 3-encoder CrossLoc net), but `forward` does not run PyTorch ops: it is
lowered once per input shape to an op list (include/crossloc_cnn.h) of hand-written HIP kernels — implicit-GEMM
convolutions on fp32 MFMA, two-pass GroupNorm with fused ReLU/residual epilogues, fused decoder head — and
executed with one C call on the current HIP stream.  NCHW at the module boundary, NHWC inside.  With autograd enabled
and trainable parameters, forward keeps the activations and `loss.backward()` runs a second op list (data
gradients through the same MFMA kernel, split-K weight gradients, fused GroupNorm/ReLU/residual backward).

The nn.Conv2d / nn.GroupNorm children are parameter containers only (they give identical keys, shapes and
default initialisation); they are never called.  There is no CPU/eager fallback: forward on a non-GPU tensor
raises.  The backward pass covers the single-task and the 3-encoder MLR networks (frozen encoders are skipped).
"""
import ctypes
import weakref

import torch
import torch.nn as nn

from . import _lib, switches
from .forms import _Forms
from .lower_backward import _BackwardLowering
from .lower_forward import _DUMMY, _ForwardLowering  # noqa: F401
from .ops import (  # noqa: F401  (the op ABI is importable from here, as it always was)
    CONV_ACCUMULATE, CONV_DGRAD, CONV_M_TILE_MAJOR, CONV_NORM_ADD, CONV_NORM_IN, CONV_NORM_RELU,
    CONV_PAIR_AMAX, CONV_PAIR_F16, CONV_SPLIT_ACT, CONV_SPLIT_BF16, CONV_SPLIT_IL, GNB_PARAMS_ITEM_DTYPE,
    GN_ACC_AUX, GN_ADD, GN_NO_CONV_BIAS, GN_RELU_IN, GN_RELU_OUT, PAIR_ITEM_DTYPE, XL_ERR_UNSUPPORTED,
    XL_OP_CONV, XL_OP_CONV1, XL_OP_CONV1_WGRAD, XL_OP_DUC_HEAD, XL_OP_DUC_HEAD_BWD, XL_OP_FILL0,
    XL_OP_GNB_APPLY, XL_OP_GNB_FINAL, XL_OP_GNB_PARAMS, XL_OP_GNB_PARAMS_LIST, XL_OP_GNB_STATS,
    XL_OP_GN_APPLY, XL_OP_GN_FINAL, XL_OP_GN_STATS, XL_OP_HEAD, XL_OP_HEAD_BWD, XL_OP_S2_DGRAD, XL_OP_STEM12,
    XL_OP_WGRAD, XL_OP_WINO_DY, XL_OP_WINO_IN, XL_OP_WINO_OUT, XL_OP_WINO_WFINAL, XlOp, _bind, _check)
from .packing import _Packing


# ------------------------------------------------------------------------------------------ parameter containers

def _create_res_block(tiny, num_gn_channel, ch_down_factor=1):
    """networks.py:133-146 (ReLU entries keep the Sequential indices 0,1,3,4,6,7 of the reference keys)."""
    num_ch = (512, 128)[tiny] // ch_down_factor
    g = min(num_gn_channel, num_ch)
    return nn.Sequential(nn.Conv2d(num_ch, num_ch, 3, 1, 1), nn.GroupNorm(g, num_ch), nn.ReLU(),
                         nn.Conv2d(num_ch, num_ch, 1, 1, 0), nn.GroupNorm(g, num_ch), nn.ReLU(),
                         nn.Conv2d(num_ch, num_ch, 3, 1, 1), nn.GroupNorm(g, num_ch), nn.ReLU())


def _create_mlr_concatenator(num_mlr, tiny, num_gn_channel):
    """networks.py:149-163"""
    cin, cout = (512, 128)[tiny] * num_mlr, (512, 128)[tiny]
    return nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1), nn.GroupNorm(num_gn_channel, cout), nn.ReLU(),
                         nn.Conv2d(cout, cout, 1, 1, 0), nn.GroupNorm(num_gn_channel, cout), nn.ReLU(),
                         nn.Conv2d(cout, cout, 3, 1, 1), nn.GroupNorm(num_gn_channel, cout), nn.ReLU())


def _create_mlr_skip_layer(num_mlr, tiny, num_gn_channel):
    """networks.py:166-172"""
    cin, cout = (512, 128)[tiny] * num_mlr, (512, 128)[tiny]
    return nn.Sequential(nn.Conv2d(cin, cout, 1, 1, 0), nn.GroupNorm(num_gn_channel, cout))


class TransPoseNetEncoder(nn.Module):
    """Parameter layout of networks.py:175-219."""

    def __init__(self, tiny, grayscale, enc_add_res_block=0, num_gn_channel=32):
        super().__init__()
        self.tiny, self.grayscale = tiny, grayscale
        self.enc_add_res_block, self.num_gn_channel = enc_add_res_block, num_gn_channel
        g = num_gn_channel
        c4, c5 = (256, 128)[tiny], (512, 128)[tiny]
        self.conv1 = nn.Conv2d(1 if grayscale else 3, g, 3, 1, 1)
        self.norm1 = nn.GroupNorm(g, g)
        self.conv2 = nn.Conv2d(g, 64, 3, 2, 1)
        self.norm2 = nn.GroupNorm(g, 64)
        self.conv3 = nn.Conv2d(64, 128, 3, 2, 1)
        self.norm3 = nn.GroupNorm(g, 128)
        self.conv4 = nn.Conv2d(128, c4, 3, 2, 1)
        self.norm4 = nn.GroupNorm(g, c4)
        self.res1_conv1 = nn.Conv2d(c4, c4, 3, 1, 1)
        self.res1_norm1 = nn.GroupNorm(g, c4)
        self.res1_conv2 = nn.Conv2d(c4, c4, 1, 1, 0)
        self.res1_norm2 = nn.GroupNorm(g, c4)
        self.res1_conv3 = nn.Conv2d(c4, c4, 3, 1, 1)
        self.res1_norm3 = nn.GroupNorm(g, c4)
        self.res2_conv1 = nn.Conv2d(c4, c5, 3, 1, 1)
        self.res2_norm1 = nn.GroupNorm(g, c5)
        self.res2_conv2 = nn.Conv2d(c5, c5, 1, 1, 0)
        self.res2_norm2 = nn.GroupNorm(g, c5)
        self.res2_conv3 = nn.Conv2d(c5, c5, 3, 1, 1)
        self.res2_norm3 = nn.GroupNorm(g, c5)
        if not tiny:
            self.res2_skip = nn.Conv2d(256, 512, 1, 1, 0)
            self.res2_skip_norm = nn.GroupNorm(g, 512)
        self.enc_add_res_block_ls = [_create_res_block(tiny, g) for _ in range(enc_add_res_block)]
        for i, block in enumerate(self.enc_add_res_block_ls):
            self.add_module('enc_add_res_block{:d}'.format(i + 1), block)


class DenseUpsamplingConvolution(nn.Module):
    """Parameter layout of networks.py:259-273 (conv 3x3 -> GroupNorm -> ReLU -> pixel shuffle x down_sampling_rate)."""

    def __init__(self, down_sampling_rate, in_channel, num_classes, num_gn_channel=32):
        super().__init__()
        self.conv = nn.Conv2d(in_channel, (down_sampling_rate ** 2) * num_classes, 3, 1, 1)
        self.norm = nn.GroupNorm(num_gn_channel, (down_sampling_rate ** 2) * num_classes)


class TransPoseNetDecoder(nn.Module):
    """Parameter layout of networks.py:276-317, including the full_size_output (DUC / semantics) branch."""

    def __init__(self, mean, tiny, dec_add_res_block=0, num_task_channel=3, num_pos_channel=1, num_gn_channel=32,
                 full_size_output=False):
        super().__init__()
        self.register_buffer('mean', mean.clone().float())
        self.tiny, self.dec_add_res_block = tiny, dec_add_res_block
        self.num_task_channel, self.num_pos_channel = num_task_channel, num_pos_channel
        self.num_gn_channel, self.full_size_output = num_gn_channel, full_size_output
        c = (512, 128)[tiny]
        g = num_gn_channel
        self.dec_add_res_block_ls = [_create_res_block(tiny, g) for _ in range(dec_add_res_block)]
        for i, block in enumerate(self.dec_add_res_block_ls):
            self.add_module('dec_add_res_block{:d}'.format(i + 1), block)
        self.res3_conv1 = nn.Conv2d(c, c, 1, 1, 0)
        self.res3_norm1 = nn.GroupNorm(g, c)
        self.res3_conv2 = nn.Conv2d(c, c, 1, 1, 0)
        self.res3_norm2 = nn.GroupNorm(g, c)
        self.res3_conv3 = nn.Conv2d(c, c, 1, 1, 0)
        self.res3_norm3 = nn.GroupNorm(g, c)
        self.fc1 = nn.Conv2d(c, c, 1, 1, 0)
        self.fc1_norm = nn.GroupNorm(min(c, g), c)
        self.fc2 = nn.Conv2d(c, c, 1, 1, 0)
        self.fc2_norm = nn.GroupNorm(min(c, g), c)
        assert num_task_channel > 0 and num_pos_channel >= 0
        assert num_task_channel == len(mean)
        if full_size_output:
            nc = num_task_channel + num_pos_channel
            self.duc_upsample = DenseUpsamplingConvolution(8, c, nc)
            self.fc3 = nn.Conv2d(nc, nc, 1, 1, 0)
        else:
            self.fc3 = nn.Conv2d(c, num_task_channel + num_pos_channel, 1, 1, 0)

# ------------------------------------------------------------------------------------------ the plan

class _Plan(_Packing, _Forms, _ForwardLowering, _BackwardLowering):
    """One pass for a fixed (B, H, W): op array + workspace, replayed on every call.

    train=False: inference plan (GroupNorm in place, buffers recycled as soon as they are dead).
    train=True:  every conv output (pre-norm) and every activation is kept, a tape of the layers is recorded and a
                 second op array for the backward pass is lowered from it (data gradients through the same
                 implicit-GEMM kernel, weight gradients, GroupNorm/epilogue backward, head backward).

    The class is assembled from its concerns: weight operands (packing.py), the choice of kernel forms (forms.py), forward
    lowering (lower_forward.py), backward lowering (lower_backward.py); construction, replay and the HIP graph are here.
    `__init__` declares every attribute a plan can carry."""

    def __init__(self, net, B, H, W, device, train=False):
        self.B, self.H, self.W, self.device, self.train = B, H, W, device, train
        self.net = net
        self.sw = switches.Snapshot()       # the lowering switches, read ONCE: both lowerings and every refresh answer from it
        # separate per-image statistics passes instead of the conv-epilogue ones (whose partial sums are grouped by
        # conv tile, i.e. by the position of a frame inside the batch): results bitwise independent of the batch
        self.separate_stats = bool(getattr(net, "batch_invariant", False) or self.sw.NO_FUSED_STATS)
        # -- workspace and weight operands
        self.keep = []                      # tensors the op pointers reference
        self.free = {}                      # numel -> [tensor]
        self.packed = {}                    # (id(param), kind) -> (packed weight tensor, source, kind)
        self.packed_split, self.packed_1x1, self.packed_c1, self.packed_pair = {}, {}, {}, {}
        self.kept_v_bytes = 0               # Winograd V tensors a training plan keeps for its weight gradients
        # the activation scales of the fp16-pair GEMMs (csrc/xl_gemm_pair.hip): {s, 1/s} for GroupNorm outputs and sums of
        # them, {s/256, 256/s} for their Winograd transforms; written by _update_pair_scales() once the plan's GroupNorm layers are
        # known, and again whenever the parameters change
        self.pair_scales = torch.zeros(8, dtype=torch.float32, device=device)
        self._unit_gn = {}                  # channels -> (ones, zeros): the affine parameters of a GroupNorm without any
        self._pair_gn, self._pair_gn_keep, self._pair_gn_sig = None, [], None       # argument table of xl_cnn_pair_scales
        self._pair_tables, self._pair_tables_sig = [], None                         # device tables of xl_cnn_repack_pairs
        # -- forward lowering
        self.ops, self.tape = [], []        # tape: one entry per layer of a training plan, read by the backward lowering
        self.max_stats = self.max_coeff = 0
        self.stats_ops = []                 # ops using the shared statistics scratch (inference)
        self.out_op_index, self.out_shape = None, None
        self.image_op_indices, self.wino_gemm_indices = [], []
        self.pending_gn = {}                # activation key -> GroupNorm apply op left to the activation's only consumer
        self.pending_entry = {}             # ... and its tape entry (training plans)
        self.pending_fold = {}              # activation key -> apply left to the first of several consumers (_fold_begin)
        self.pending_aux = {}               # activation key -> apply of a residual, left to the pass that adds it (_aux_defer)
        self.pending_res = {}               # activation key -> residual tensor of a deferred apply-and-add
        self.held = {}                      # id(tensor) -> [tensor, released meanwhile]: inputs of an apply not yet emitted
        self.deferred_gn_consumers = []     # ops reading the shared coefficient table as aux2
        self.aux_final_ops, self.aux_apply_ops, self.aux_coef_consumers, self.coeff_aux = [], [], [], None      # ... and the second table
        # -- backward lowering (training plans)
        self.pair_bwd, self.bwd_array, self.bwd_amax, self.bwd_scratch_f, self.bwd_scratch_d = False, None, None, None, None
        self.grad_flat, self.grad_slices, self.param_grads = None, [], []     # (parameter, offset, numel) / (parameter, slice)
        self.head_bwd_index, self.conv1_wgrad_indices, self.gnb_params_table, self.conv1_db_unused = None, [], None, None
        # -- replay
        self.last_image = self.last_out = None
        self.grad_results, self.grad_turn = [None, None], 0
        self.busy, self.generation = False, 0            # a training plan holds the activations of one autograd graph
        self.graph = self.graph_in = self.graph_out = self.graph_stream = self.graph_private = None
        self.graph_runs, self.graph_off, self.graph_on_null_stream = 0, False, True

        self._lower(net)
        self._update_pair_scales()
        self.op_array = (XlOp * len(self.ops))(*self.ops)
        self.stats = torch.zeros(max(self.max_stats, 1), dtype=torch.float64, device=device)
        for i in self.stats_ops:
            self.op_array[i].stats = self.stats.data_ptr()
        self.coeff = torch.zeros(max(self.max_coeff, 1), dtype=torch.float32, device=device)
        for i, op in enumerate(self.ops):
            # every GN_FINAL writes the shared coefficient buffer; its consumer - the following GN_APPLY, or the
            # Winograd input transform of the next layer when the apply was deferred - runs before the next GN_FINAL
            if op.type == XL_OP_GN_FINAL and not train:
                self.op_array[i].out = self.coeff.data_ptr()
            elif op.type == XL_OP_GN_APPLY and not train:
                self.op_array[i].aux2 = self.coeff.data_ptr()
        for i in self.deferred_gn_consumers:
            self.op_array[i].aux2 = self.coeff.data_ptr()
        if self.aux_final_ops:              # the second table: residuals normalised by the pass that adds them
            self.coeff_aux = torch.zeros_like(self.coeff)
            for i in self.aux_final_ops:
                self.op_array[i].out = self.coeff_aux.data_ptr()
            for i in self.aux_apply_ops:
                self.op_array[i].aux2 = self.coeff_aux.data_ptr()
            for i in self.aux_coef_consumers:
                self.op_array[i].w = self.coeff_aux.data_ptr()
        assert not self.pending_gn, "a deferred GroupNorm was never consumed"
        assert not self.pending_aux, "a deferred residual GroupNorm was never consumed"
        assert not self.pending_fold, "a folded GroupNorm apply was never consumed"
        if train:
            self._lower_backward()
            self._update_pair_scales()          # (the backward GEMMs may be the plan's first pair operands: small maps)

    GRAPH_MAX_BATCH = 8            # plans of at most this many frames replay their op list as one HIP graph (XL_CNN_GRAPH)

    def _graph_wanted(self, stream):
        env = switches.live("XL_CNN_GRAPH")
        if self.train or env == "0":
            return False
        return env == "1" or self.B <= self.GRAPH_MAX_BATCH

    def _run_graph(self, image, stream):
        """Latency path: the ~95 launches of a small-batch forward as one executable HIP graph.  The graph holds pointers,
        so the image is copied into a buffer of the plan (4 MB per frame, one device-to-device copy) and the result is
        handed out as a copy of the plan's result buffer.  Returns None when the eager path has to run (first call of the
        plan: every kernel configures itself on its first launch; per-op profiling)."""
        L = _bind()
        if self.graph_in is None:
            self.graph_in = torch.empty_like(image)
            self.graph_out = torch.empty(self.out_shape, dtype=torch.float32, device=self.device)
        if self.graph_off:
            return None
        self.graph_runs += 1
        if self.graph_runs == 1:
            return None                                     # warm-up: eager
        # one stream per plan: the graph's input / result buffers belong to the plan, and a launch on another stream could
        # overlap the copy-in of the next call or the copy-out of this one (callers that drive one network from several
        # streams pass distinct plan_slots).  A call from any other stream than the capturing one runs eagerly.
        if self.graph_stream is not None and stream != self.graph_stream:
            return None
        # round 5: the caller is on the DEFAULT stream - what the reference's unchanged loop uses (test_single_task.py:347,
        # `network(image.cuda())`), and a stream HIP cannot capture on.  The graph then lives on a private stream of the plan,
        # bracketed by events: copy-in on the caller's stream, graph behind it, the result copy back on the caller's stream
        # behind the graph.  Same kernels, same order, same bits as the eager op list.
        private = None
        if stream == 0:
            if self.graph_private is None:
                self.graph_private = torch.cuda.Stream(device=self.device)
            private = self.graph_private
        for i in self.image_op_indices:
            self.op_array[i].in_ = self.graph_in.data_ptr()
        self.op_array[self.out_op_index].out = self.graph_out.data_ptr()
        if self.graph is None:
            h = ctypes.c_void_p()
            rc = L.xl_cnn_graph_capture(self.op_array, len(self.op_array),
                                        ctypes.c_void_p(private.cuda_stream if private is not None else stream), ctypes.byref(h))
            if rc != 0:
                return self._graph_give_up("capture", rc)
            self.graph, self.graph_stream = h, stream
            weakref.finalize(self, L.xl_cnn_graph_destroy, h)
        self.graph_in.copy_(image)
        if private is not None and not self.graph_on_null_stream:
            caller = torch.cuda.current_stream()
            private.wait_stream(caller)                     # the copy-in (and whatever produced the image) before the graph
            rc = L.xl_cnn_graph_launch(self.graph, ctypes.c_void_p(private.cuda_stream))
            caller.wait_stream(private)                     # the caller's next operation - the result copy - behind the graph
        elif private is not None:
            # round 6: a graph CAPTURED on the private stream may be LAUNCHED on the default stream - only capture is refused
            # there - so the copy-in, the graph and the result copy are simply in stream order: no events, four driver calls
            # fewer per frame.  A runtime that refuses falls back to the bracketed form for the life of the plan.
            rc = L.xl_cnn_graph_launch(self.graph, ctypes.c_void_p(0))
            if rc != 0 and rc != XL_ERR_UNSUPPORTED:
                self.graph_on_null_stream = False
                self.graph_runs -= 1                         # (this call was counted already)
                return self._run_graph(image, stream)
        else:
            rc = L.xl_cnn_graph_launch(self.graph, ctypes.c_void_p(stream))
        if rc == XL_ERR_UNSUPPORTED:                        # per-op profiling is on: this call runs eagerly
            return None
        if rc != 0:
            return self._graph_give_up("launch", rc)
        return self.graph_out.clone()

    def _graph_give_up(self, what, rc):
        """A capture / launch failure must not make small-batch inference unusable where the eager path works (a call inside the
        op list that cannot be captured, e.g. a first-use hipFuncSetAttribute on another device): say so once, stop trying."""
        import warnings
        L = _lib.lib()
        warnings.warn("crossloc_amd: HIP-graph %s of a %d-frame plan failed (%s %s); this plan runs its op list eagerly from now on"
                      % (what, self.B, L.xl_status_string(rc).decode(), L.xl_cnn_last_error().decode()))
        self.graph_off = True
        return None

    def run(self, image):
        stream = torch.cuda.current_stream().cuda_stream
        if self._graph_wanted(stream):
            out = self._run_graph(image, stream)
            if out is not None:
                self.last_image, self.last_out = image, out.detach()
                return out
        out = torch.empty(self.out_shape, dtype=torch.float32, device=self.device)
        for i in self.image_op_indices:
            self.op_array[i].in_ = image.data_ptr()
        self.op_array[self.out_op_index].out = out.data_ptr()
        _check(_bind().xl_cnn_run(self.op_array, len(self.op_array), ctypes.c_void_p(stream)))
        # (a detached alias: the returned tensor itself becomes the output of the autograd node in training, and a
        # reference to it from here would keep that graph - and the plan's busy token - alive)
        self.last_image, self.last_out = image, out.detach()
        return out

    def run_backward(self, dout):
        """dout [B, Cout, Ho, Wo] (NCHW, like the forward output).  Returns [(parameter, flat gradient)]."""
        dout = dout.detach().to(torch.float32).contiguous()
        hb = self.bwd_array[self.head_bwd_index]
        hb.aux, hb.aux2 = dout.data_ptr(), self.last_out.data_ptr()
        for i in self.conv1_wgrad_indices:
            self.bwd_array[i].in_ = self.last_image.data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
        _check(_bind().xl_cnn_run(self.bwd_array, len(self.bwd_array), ctypes.c_void_p(stream)))
        # hand the gradients out as slices of a copy of the flat buffer (ONE device-to-device copy; the plan's own buffer
        # is overwritten by the next backward pass).  Two result buffers alternate - their addresses repeat, which keeps
        # the fused optimizer's pointer table valid - but a buffer is reused only when NOTHING else references its
        # storage any more: a .grad that is still alive (accumulation without zero_grad), a result of torch.autograd.grad,
        # a tensor kept by a hook or for logging all hold a view, and then a fresh buffer is handed out instead.
        self.grad_turn ^= 1
        buf = self.grad_results[self.grad_turn]
        if buf is not None and not _sole_owner(buf):
            buf = None
        if buf is None:
            buf = self.grad_results[self.grad_turn] = torch.empty_like(self.grad_flat)
        buf.copy_(self.grad_flat)
        return [(p, buf[o:o + n]) for p, o, n in self.grad_slices]


def gradient_buffer(net):
    """The flat fp32 buffer that the `.grad` of every trainable parameter of `net` is a slice of after a backward pass
    (run_backward hands the gradients out as views of one result buffer).  One in-place collective on it reduces every
    gradient at once.  Raises when the gradients are not the ones the last backward produced (missing, accumulated into a
    tensor of their own, or replaced).  The caller must not keep the buffer across steps: a live view pins it (_sole_owner)."""
    params = [p for p in net._tensors()[0] if p.requires_grad]
    if not params or params[0].grad is None:
        raise RuntimeError("gradient_buffer: no gradients (call it between loss.backward() and optimizer.zero_grad())")
    ptr = params[0].grad.untyped_storage().data_ptr()
    for plan in net._plans.values():
        for buf in plan.grad_results:
            if buf is None or buf.data_ptr() != ptr:
                continue
            if len(plan.grad_slices) != len(params) or any(
                    p.grad is None or p.grad.data_ptr() != ptr + 4 * o for p, o, _ in plan.grad_slices):
                break
            return buf
    raise RuntimeError("gradient_buffer: the .grad tensors are not the slices of one backward result buffer")


def _sole_owner(buf):
    """True when `buf` is the only tensor left on its storage (no view of it is alive anywhere): 2 = this tensor + the
    Python storage object the query itself creates.  Unknown (private API missing) counts as shared."""
    try:
        return torch._C._storage_Use_Count(buf.untyped_storage()._cdata) <= 2
    except (AttributeError, RuntimeError, TypeError):
        if not getattr(_sole_owner, "warned", False):
            _sole_owner.warned = True
            import warnings
            warnings.warn("crossloc_amd: torch._C._storage_Use_Count is unavailable in this PyTorch: every backward pass allocates a fresh "
                          "gradient buffer (correct, but the fused optimizer rebuilds its pointer tables each step)")
        return False


class _NetFunction(torch.autograd.Function):
    """Connects the HIP forward/backward plans to autograd: the parameters are passed as inputs so that
    `loss.backward()` (train_single_task.py:298) routes the output gradient into run_backward and accumulates the
    returned parameter gradients into `.grad` like any other op.  The image gradient is not computed."""

    @staticmethod
    def forward(ctx, plan, x, *params):
        ctx.plan, ctx.params = plan, params
        out = plan.run(x)
        # the plan's buffers hold this graph's activations until its backward ran or the graph is dropped
        plan.generation = gen = plan.generation + 1
        plan.busy = True
        ctx.generation = gen
        ctx.token = _Token()
        weakref.finalize(ctx.token, _release_plan, weakref.ref(plan), gen)
        return out

    @staticmethod
    def backward(ctx, gout):
        if ctx.generation != ctx.plan.generation:
            raise RuntimeError("the activations of this graph were overwritten by a later forward of the same plan "
                               "(backward twice through one graph after another forward?)")
        produced = {id(p): g for p, g in ctx.plan.run_backward(gout)}
        ctx.plan.busy = False
        grads = tuple(produced[id(p)].view_as(p) if (p.requires_grad and id(p) in produced) else None
                      for p in ctx.params)
        return (None, None) + grads


class _Token:
    """Lives as long as the autograd node of one training forward (see _NetFunction.forward)."""


def _release_plan(plan_ref, generation):
    plan = plan_ref()
    if plan is not None and plan.generation == generation:
        plan.busy = False


class TransPoseNet(nn.Module):
    """Drop-in for networks.py:362-502.  forward(inputs[B,C,H,W] on the GPU) -> [B, n_task+n_pos, H/8, W/8], or
    [B, n_task+n_pos, H, W] with full_size_output (the DUC / semantics head, inference only)."""

    def __init__(self, mean, tiny, grayscale, enc_add_res_block=0, dec_add_res_block=0, num_task_channel=3,
                 num_pos_channel=1, num_gn_channel=32, num_mlr=0, num_unfrozen_encoder=0, full_size_output=False):
        super().__init__()
        # True: inference / training plans run separate per-image GroupNorm statistics passes, which makes every frame's
        # result bitwise independent of the batch it is in (default: conv-epilogue statistics, ~4 % faster, equal to
        # the last fp32 bit or two).  Set before the first forward.
        self.batch_invariant = False
        mean = torch.as_tensor(mean, dtype=torch.float32)
        self.register_buffer('mean', mean.clone())
        self.tiny, self.grayscale = tiny, grayscale
        self.enc_add_res_block, self.dec_add_res_block = enc_add_res_block, dec_add_res_block
        self.num_task_channel, self.num_pos_channel = num_task_channel, num_pos_channel
        self.num_gn_channel, self.num_mlr, self.full_size_output = num_gn_channel, num_mlr, full_size_output
        self.OUTPUT_SUBSAMPLE = 1 if full_size_output else 8
        if num_mlr == 0:
            self.encoder = TransPoseNetEncoder(tiny, grayscale, enc_add_res_block, num_gn_channel)
            self.encoder_ls = [self.encoder]
            self.mlr_encoder_ls = [nn.Identity()]
            self.mlr_norm, self.mlr_forward, self.mlr_skip = nn.Identity(), nn.Identity(), nn.Identity()
        else:
            assert isinstance(num_mlr, int) and 0 <= num_unfrozen_encoder <= num_mlr
            self.encoder = nn.Identity()
            self.encoder_ls = [self.encoder]
            self.mlr_encoder_ls = [TransPoseNetEncoder(tiny, grayscale, enc_add_res_block, num_gn_channel)
                                   for _ in range(num_mlr)]
            for i, block in enumerate(self.mlr_encoder_ls):
                if i >= num_unfrozen_encoder:                       # networks.py:424-428
                    for p in block.parameters():
                        p.requires_grad = False
                self.add_module('mlr_encoder_{:d}'.format(i + 1), block)
            self.mlr_norm = nn.GroupNorm(num_gn_channel, (512, 128)[tiny] * num_mlr)
            self.mlr_forward = _create_mlr_concatenator(num_mlr, tiny, num_gn_channel)
            self.mlr_skip = _create_mlr_skip_layer(num_mlr, tiny, num_gn_channel)
        self.decoder = TransPoseNetDecoder(mean, tiny, dec_add_res_block, num_task_channel, num_pos_channel,
                                           num_gn_channel, full_size_output)
        self.decoder_ls = [self.decoder]
        self._plans = {}
        self._plan_version = None

    def _tensors(self):
        """(parameters, version) - the parameter list of the module tree and the sum of all parameter / buffer version counters.
        `nn.Module.parameters()` / `.buffers()` walk the tree with de-duplicating generators: 0.35 ms of host time per forward for
        this network, a sixth of a single frame's 2 ms in the reference's per-frame loop; the cached (owner, name, tensor) triples
        cost 0.02.  What the cache guarantees: every call re-checks each cached slot by identity - a dictionary look-up per
        tensor - so a parameter or buffer REPLACED on a module the cache knows (`mod.weight = nn.Parameter(...)`,
        `load_state_dict(assign=True)`) rebuilds it, and `.to()` / `load_state_dict` drop it.  What it does not see: a submodule
        that was replaced or added after the first forward (the old module still holds its old tensors, so its slots still
        match); call `net.__dict__.pop("_tensor_cache", None)` and `net.invalidate()` after such surgery."""
        cache = self.__dict__.get("_tensor_cache")
        if cache is not None:
            ver = 0
            for owner, name, t, is_param in cache:
                if (owner._parameters if is_param else owner._buffers).get(name) is not t:
                    cache = None
                    break
                ver += t._version
            if cache is not None:
                return self.__dict__["_param_list"], ver
        cache, seen = [], set()
        for mod in self.modules():
            for name, t in mod._parameters.items():
                if t is not None and id(t) not in seen:
                    seen.add(id(t)); cache.append((mod, name, t, True))
            for name, t in mod._buffers.items():
                if t is not None and id(t) not in seen:
                    seen.add(id(t)); cache.append((mod, name, t, False))
        self.__dict__["_tensor_cache"] = cache
        self.__dict__["_param_list"] = list(self.parameters())            # (the order autograd's inputs are bound in)
        return self.__dict__["_param_list"], sum(t._version for _, _, t, _ in cache)

    def _version(self):
        return self._tensors()[1]

    def invalidate(self):
        """Drop cached plans (packed weights); called automatically when a parameter changes in place."""
        self._plans = {}

    def _apply(self, fn, *a, **k):
        self._plans = {}
        self.__dict__.pop("_tensor_cache", None)
        return super()._apply(fn, *a, **k)

    def drop_plans_except(self, B, H, W):
        """Release the plans (activation buffers, packed operands) of every input shape but [B, *, H, W] - a training loop
        whose augmentation changes the input size from batch to batch keeps one size's plans at a time.  Plans that hold
        the activations of a graph not yet differentiated stay."""
        for k in [k for k, p in self._plans.items() if tuple(k[:3]) != (B, H, W) and not p.busy]:
            del self._plans[k]

    def load_state_dict(self, *a, **k):
        self._plans = {}
        self.__dict__.pop("_tensor_cache", None)
        return super().load_state_dict(*a, **k)

    def forward(self, inputs, plan_slot=0):
        """plan_slot: calls that may be in flight at the same time on different HIP streams (evaluation.PipelinedLocalizer
        runs two half-batches concurrently) must use different slots: a plan owns its activation buffers."""
        if not isinstance(inputs, torch.Tensor) or inputs.dim() != 4:
            raise RuntimeError("TransPoseNet.forward expects a 4D tensor [B,C,H,W]")
        if not inputs.is_cuda:
            raise RuntimeError("crossloc_amd.TransPoseNet runs on the MI355X only (no CPU fallback); got a CPU tensor")
        x = inputs.detach().to(torch.float32).contiguous()
        B, C, H, W = x.shape
        if C != (1 if self.grayscale else 3):
            raise RuntimeError("expected %d input channels, got %d" % (1 if self.grayscale else 3, C))
        params, ver = self._tensors()
        if ver != self._plan_version:
            for plan in self._plans.values():
                plan.refresh_weights()
            self._plan_version = ver
        train = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        # The conv kernel addresses a tensor with 32-bit byte offsets; inference launches whose tensors pass 2 GiB (the
        # 32-channel full-resolution activation does at 48 frames of 480x720) are issued per image range inside the
        # library (launch_igemm), so inference batches have no limit here.  The backward kernels are not segmented.
        max_b = max(1, (2 ** 31 - 1) // (H * W * self.num_gn_channel * 4) - 1)
        if B > max_b and train:
            raise RuntimeError("training batch of %d frames exceeds the per-launch limit of %d at %dx%d" % (B, max_b, H, W))
        key = (B, H, W, x.device.index, train) if plan_slot == 0 else (B, H, W, x.device.index, train, plan_slot)
        if self.batch_invariant:
            key = key + ("batch_invariant",)
        with torch.cuda.device(x.device):
            plan = self._plans.get(key)
            if plan is None:
                plan = _Plan(self, B, H, W, x.device, train=train)
                self._plans[key] = plan
            if not train:
                return plan.run(x)
            # a training plan holds the activations of ONE graph until its backward ran (or the graph was dropped): a
            # second grad-enabled forward before that (gradient accumulation over two forwards, two losses) gets a
            # plan of its own instead of silently overwriting the first graph's activations
            n = 0
            while plan.busy:
                n += 1
                if n >= 4:
                    raise RuntimeError("4 training forwards of shape %s are outstanding without a backward; run "
                                       "inference under torch.no_grad()" % (tuple(x.shape),))
                k2 = key + ("outstanding", n)
                plan = self._plans.get(k2)
                if plan is None:
                    plan = self._plans[k2] = _Plan(self, B, H, W, x.device, train=True)
            return _NetFunction.apply(plan, x, *params)
