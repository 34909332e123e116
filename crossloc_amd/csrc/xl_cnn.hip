// xl_cnn.hip — the C ABI of the scene-coordinate CNN (include/crossloc_cnn.h): xl_cnn_run executes an op list on a stream, eagerly
// or captured once as a HIP graph, with optional per-op event timing.  What PyTorch dispatched for TransPoseNet.forward and
// loss.backward() is a list of xl_op records; every op type has a launcher (xl_launch.h) in the file of its kernel family:
//
//   XL_OP_CONV1                          xl_conv1.hip       3x3 s1 on the NCHW image -> NHWC: direct, fused and matrix-pipe forms
//   XL_OP_CONV                           xl_igemm.hip       the dispatch; implicit GEMM on exact-fp32 MFMA (fallbacks, data gradients)
//                                        xl_gemm_split.hip, xl_gemm_pair.hip      1x1 and Winograd GEMMs on the bf16 / fp16 matrix pipe;
//                                                                                 one launcher of the 1x1 forms (xl_conv1x1.h)
//                                        xl_stem_split.hip, xl_stem_pair.hip      the 3x3 stride-2 stem convolutions on those pipes:
//                                                                                 one loop (xl_stem_s2.h, xl_stem_s2_body.h), two forms
//   XL_OP_STEM12, XL_OP_S2_DGRAD         xl_stem_fused.hip, xl_stem_dgrad.hip
//   XL_OP_WINO_IN, XL_OP_WINO_OUT        xl_wino.hip        Winograd F(2x2), F(4x4), F(6x6) input / output transforms
//   XL_OP_GN_STATS, _FINAL, _APPLY       xl_gn.hip          GroupNorm: fp64 partial sums, per-channel scale / shift, apply
//   XL_OP_HEAD, XL_OP_DUC_HEAD           xl_gn.hip          fc3 + mean offset + exp(hardtanh), NCHW out
//   XL_OP_WGRAD                          xl_wgrad_f32.hip   the dispatch; exact-fp32 split-K kernel and the reduce over the splits
//                                        xl_wgrad_split.hip, xl_wgrad_pair.hip    the products on the matrix pipes (one loop: xl_wgrad.h, xl_wgrad_body.h)
//   XL_OP_WINO_DY, XL_OP_WINO_WFINAL     xl_wgrad_f32.hip   the transforms around the batched weight-gradient products of a Winograd layer
//   XL_OP_GNB_* (five)                   xl_gn_bwd.hip      GroupNorm backward fused with the forward epilogue; d gamma / d beta / d bias
//   XL_OP_HEAD_BWD, XL_OP_DUC_HEAD_BWD   xl_head_bwd.hip
//   XL_OP_CONV1_WGRAD                    xl_conv1.hip       behind the forward forms
//   XL_OP_FILL0                          here: a hipMemsetAsync
//
// The weight packs of all of them are in xl_pack.hip.  fp32 end to end: the MFMA forms are bitwise fmaf chains or exact
// splits, so parity with the fp32 reference is at summation-order level.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "xl_launch.h"

namespace {

thread_local char g_err[256] = "";

// ---- optional per-op HIP-event timing (bench.py roofline leg): events are recorded on the launch stream
// around every op while profiling is on, and resolved after the caller has synchronised.
struct ProfRec { hipEvent_t a, b; int opIndex; int type; };
ProfRec *g_prof = nullptr;
int g_profCap = 0, g_profCount = 0;
bool g_profOn = false;
int g_profType = -1, g_profMinBatched = 0;     // record only ops of this type (-1: all) with nchunks2 >= the minimum

int run_op(const xl_op &op, hipStream_t st)
{
    switch (op.type) {
        case XL_OP_CONV1: return xl_run_conv1(op, st);
        case XL_OP_CONV: return xl_run_conv(op, st);
        case XL_OP_STEM12: return xl_run_stem12(op, st);
        case XL_OP_S2_DGRAD: return xl_run_s2_dgrad(op, st);
        case XL_OP_WINO_IN: return xl_run_wino_in(op, st);
        case XL_OP_WINO_OUT: return xl_run_wino_out(op, st);
        case XL_OP_GN_STATS: return xl_run_gn_stats(op, st);
        case XL_OP_GN_APPLY: return xl_run_gn_apply(op, st);
        case XL_OP_GN_FINAL: return xl_run_gn_final(op, st);
        case XL_OP_HEAD: return xl_run_head(op, st);
        case XL_OP_DUC_HEAD: return xl_run_duc_head(op, st);
        case XL_OP_FILL0:                                 // `Cin` bytes at `out` set to zero on the stream
            if (!op.out || op.Cin < 1) return XL_ERR_ARG;
            return hipMemsetAsync(op.out, 0, (size_t)op.Cin, st) == hipSuccess ? XL_OK : XL_ERR_HIP;
        case XL_OP_WGRAD: return xl_run_wgrad(op, st);
        case XL_OP_WINO_DY: return xl_run_wino_dy(op, st);
        case XL_OP_WINO_WFINAL: return xl_run_wino_wfinal(op, st);
        case XL_OP_GNB_STATS:
        case XL_OP_GNB_FINAL:
        case XL_OP_GNB_APPLY: return xl_run_gnb(op, st);
        case XL_OP_GNB_PARAMS: return xl_run_gnb_params(op, st);
        case XL_OP_GNB_PARAMS_LIST: return xl_run_gnb_params_list(op, st);
        case XL_OP_HEAD_BWD: return xl_run_head_bwd(op, st);
        case XL_OP_DUC_HEAD_BWD: return xl_run_duc_head_bwd(op, st);
        case XL_OP_CONV1_WGRAD: return xl_run_conv1_wgrad(op, st);
        default: return XL_ERR_UNSUPPORTED;
    }
}

}  // namespace

void xl_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" {

// which op of a list a launcher refused (the launchers return a bare status): read back through xl_cnn_last_error()
static void note_failed_op(const xl_op &op, int index, int rc)
{
    (void)rc;
    char why[160];
    snprintf(why, sizeof(why), "%s", g_err);                              // (a launcher's own text - cleared at the head of the list - stays in front)
    snprintf(g_err, sizeof(g_err), "%s%sop %d refused (type %d, k%d s%d, %d -> %d channels, in %dx%d out %dx%d, B %d, ld %d/%d, flags 0x%x, Z %d, form %d)",
             why, why[0] ? "; " : "", index, op.type, op.ksize, op.stride, op.Cin, op.Cout, op.Hi, op.Wi, op.Ho, op.Wo, op.B, op.ld_in, op.ld_out,
             (unsigned)op.flags, op.nchunks2, op.reserved_i);
}

int xl_cnn_run(const xl_op *ops, int n_ops, void *stream)
{
    if (!ops || n_ops < 0) return XL_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    g_err[0] = 0;
    for (int i = 0; i < n_ops; ++i) {
        const bool rec = g_profOn && g_profCount < g_profCap && (g_profType < 0 || ops[i].type == g_profType) &&
                         ops[i].nchunks2 >= g_profMinBatched;
        if (rec) (void)hipEventRecord(g_prof[g_profCount].a, st);
        const int rc = run_op(ops[i], st);
        if (rc != XL_OK) { note_failed_op(ops[i], i, rc); return rc; }
        if (rec) {
            (void)hipEventRecord(g_prof[g_profCount].b, st);
            g_prof[g_profCount].opIndex = i; g_prof[g_profCount].type = ops[i].type;
            ++g_profCount;
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "kernel launch: %s", hipGetErrorString(e)); return XL_ERR_HIP; }
    return XL_OK;
}

int xl_cnn_op_size(void) { return (int)sizeof(xl_op); }

// ---- the op list of a plan as ONE executable HIP graph (latency path: a single frame is ~95 short launches, and the host
// side of an eager launch costs about as much as the shortest kernels run)
int xl_cnn_graph_capture(const xl_op *ops, int n_ops, void *stream, void **graph_out)
{
    if (!ops || n_ops < 1 || !stream || !graph_out) return XL_ERR_ARG;     // (the NULL stream cannot be captured)
    hipStream_t st = (hipStream_t)stream;
    const bool prof = g_profOn;
    g_profOn = false;                                                      // event records are not part of a graph
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) { g_profOn = prof; return XL_ERR_HIP; }
    g_err[0] = 0;
    int rc = XL_OK;
    for (int i = 0; i < n_ops && rc == XL_OK; ++i) {
        rc = run_op(ops[i], st);
        if (rc != XL_OK) note_failed_op(ops[i], i, rc);
    }
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    g_profOn = prof;
    if (rc != XL_OK || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        if (rc == XL_OK) snprintf(g_err, sizeof(g_err), "hipStreamEndCapture: %s", hipGetErrorString(e));
        return rc != XL_OK ? rc : XL_ERR_HIP;
    }
    hipGraphExec_t ex = nullptr;
    const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess || !ex) { snprintf(g_err, sizeof(g_err), "hipGraphInstantiate: %s", hipGetErrorString(ei)); return XL_ERR_HIP; }
    *graph_out = (void *)ex;
    return XL_OK;
}

int xl_cnn_graph_launch(void *graph, void *stream)
{
    if (!graph) return XL_ERR_ARG;
    if (g_profOn) return XL_ERR_UNSUPPORTED;                               // per-op timing needs the eager path
    const hipError_t e = hipGraphLaunch((hipGraphExec_t)graph, (hipStream_t)stream);
    if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "hipGraphLaunch: %s", hipGetErrorString(e)); return XL_ERR_HIP; }
    return XL_OK;
}

int xl_cnn_graph_destroy(void *graph)
{
    if (!graph) return XL_OK;
    return hipGraphExecDestroy((hipGraphExec_t)graph) == hipSuccess ? XL_OK : XL_ERR_HIP;
}
const char *xl_cnn_last_error(void) { return g_err; }

int xl_cnn_prof_begin(int max_records)
{
    if (max_records <= 0) return XL_ERR_ARG;
    if (g_prof) return XL_ERR_ARG;
    g_prof = (ProfRec *)calloc((size_t)max_records, sizeof(ProfRec));
    if (!g_prof) return XL_ERR_ARG;
    for (int i = 0; i < max_records; ++i) {
        if (hipEventCreate(&g_prof[i].a) != hipSuccess || hipEventCreate(&g_prof[i].b) != hipSuccess) return XL_ERR_HIP;
    }
    g_profCap = max_records; g_profCount = 0; g_profOn = true;
    return XL_OK;
}

int xl_cnn_prof_pause(int on) { g_profOn = (on != 0) && g_prof; return XL_OK; }

int xl_cnn_prof_filter(int op_type, int min_nchunks2) { g_profType = op_type; g_profMinBatched = min_nchunks2; return XL_OK; }

int xl_cnn_prof_end(int32_t *op_index, int32_t *op_type, float *ms, int capacity)
{
    if (!g_prof) return XL_ERR_ARG;
    g_profOn = false;
    int n = g_profCount < capacity ? g_profCount : capacity;
    for (int i = 0; i < n; ++i) {
        float t = 0.f;
        if (hipEventSynchronize(g_prof[i].b) != hipSuccess || hipEventElapsedTime(&t, g_prof[i].a, g_prof[i].b) != hipSuccess) t = -1.f;
        if (op_index) op_index[i] = g_prof[i].opIndex;
        if (op_type) op_type[i] = g_prof[i].type;
        if (ms) ms[i] = t;
    }
    for (int i = 0; i < g_profCap; ++i) { (void)hipEventDestroy(g_prof[i].a); (void)hipEventDestroy(g_prof[i].b); }
    free(g_prof); g_prof = nullptr; g_profCap = 0; g_profCount = 0;
    return n;
}

}  // extern "C"
