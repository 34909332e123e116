// The launcher interface between the translation units of the CNN op list: xl_cnn_run (xl_cnn.hip) hands every op to the
// launcher of its type.  A launcher checks the op before it makes any HIP call and refuses it with XL_ERR_ARG or
// XL_ERR_UNSUPPORTED (tests/test_cnn_refusals_cpu.py), or enqueues its kernels on the stream and returns XL_OK.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/crossloc_cnn.h"
#include "../../include/crossloc_dsac.h"   // status codes
#include "xl_common.h"

int xl_run_conv1(const xl_op &op, hipStream_t st);        // xl_conv1.hip
int xl_run_conv(const xl_op &op, hipStream_t st);         // xl_igemm.hip: the dispatch of XL_OP_CONV, fp32 implicit GEMM
int xl_run_split_gemm(const xl_op &op, hipStream_t st);   // xl_gemm_split.hip
int xl_run_pair(const xl_op &op, hipStream_t st);         // xl_gemm_pair.hip
int xl_run_split_stem(const xl_op &op, hipStream_t st);   // xl_stem_split.hip
int xl_run_pair_stem(const xl_op &op, hipStream_t st);    // xl_stem_pair.hip
int xl_run_stem12(const xl_op &op, hipStream_t st);       // xl_stem_fused.hip
int xl_run_s2_dgrad(const xl_op &op, hipStream_t st);     // xl_stem_dgrad.hip
int xl_run_wino_in(const xl_op &op, hipStream_t st);      // xl_wino.hip
int xl_run_wino_out(const xl_op &op, hipStream_t st);
int xl_run_gn_stats(const xl_op &op, hipStream_t st);     // xl_gn.hip
int xl_run_gn_apply(const xl_op &op, hipStream_t st);
int xl_run_gn_final(const xl_op &op, hipStream_t st);
int xl_run_head(const xl_op &op, hipStream_t st);
int xl_run_duc_head(const xl_op &op, hipStream_t st);
int xl_run_wgrad(const xl_op &op, hipStream_t st);        // xl_wgrad_f32.hip: the dispatch of XL_OP_WGRAD, fp32 kernel, reduce
int xl_run_wgrad_split(const xl_op &op, hipStream_t st);  // xl_wgrad_split.hip
int xl_run_wgrad_pair(const xl_op &op, hipStream_t st);   // xl_wgrad_pair.hip
int xl_run_wino_dy(const xl_op &op, hipStream_t st);      //   ... and the Winograd transforms around its batched products
int xl_run_wino_wfinal(const xl_op &op, hipStream_t st);
int xl_run_gnb(const xl_op &op, hipStream_t st);          // xl_gn_bwd.hip: XL_OP_GNB_STATS, _FINAL and _APPLY
int xl_run_gnb_params(const xl_op &op, hipStream_t st);
int xl_run_gnb_params_list(const xl_op &op, hipStream_t st);
int xl_run_head_bwd(const xl_op &op, hipStream_t st);     // xl_head_bwd.hip
int xl_run_duc_head_bwd(const xl_op &op, hipStream_t st);
int xl_run_conv1_wgrad(const xl_op &op, hipStream_t st);  // xl_conv1.hip

// a launcher's own words in front of the "op N refused (...)" of xl_cnn_last_error() (xl_cnn.hip, per thread)
void xl_set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

// workgroups of a grid-stride launch: one per `per` items, at most `cap`
inline unsigned xl_grid(long long items, int per, long long cap)
{
    const long long blocks = (items + per - 1) / per;
    return (unsigned)(blocks > cap ? cap : blocks);
}

// workgroups of a persistent launch over `tiles` tiles: one per CU (`resident` of them fit the chip), or, for less work, the
// tile count rounded up to a multiple of the 8 XCDs (the kernels hand every XCD a contiguous run of tiles)
inline int xl_persistent_grid(int tiles, int resident = 256)
{
    const int rounds = (tiles + 7) & ~7;
    return resident > rounds ? rounds : resident;
}
