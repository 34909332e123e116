/*
 * tests/pose_quality_oracle_ne.c — TEST INFRASTRUCTURE ONLY.  The oracle's own normal equations (xo_normal_eq of
 * oracle/dsac_oracle.c, the serial restatement of normal_eq_thread + block_sum in xl_dsac.hip) at a given pose over the
 * inlier set the refinement would form there (clamped float error < thr).  The oracle keeps that function static, so this file
 * compiles the oracle's translation unit and adds one entry point; tests/test_pose_quality_cpu.py holds the first 28 sums of the
 * pose-quality pass to its result bit for bit.  Both sides accumulate pnp_cell_normal_eq of xl_dsac_math.h per inlier, so the
 * comparison is of what surrounds it: the inlier set, the walk of the threads over the cells and the order of the additions.
 */
#include "../oracle/dsac_oracle.c"

int xq_oracle_normal_eq(const float *coords, int64_t sc, int64_t sy, int64_t sx, int Ho, int Wo, const double *Rt12,
                        float thr, float focal, float ppx, float ppy, float alpha, float maxReproj, int sub, double *out28)
{
    if (!coords || !Rt12 || !out28 || Ho <= 0 || Wo <= 0 || sub <= 0) return -1;
    xo_coords co = { coords, sc, sy, sx, Ho, Wo };
    const Cam cam = xo_cam(Ho, Wo, thr, focal, ppx, ppy, alpha, maxReproj, sub);
    Pose pose;
    pose_load12(Rt12, &pose);
    unsigned char *inl = (unsigned char *)malloc((size_t)cam.N);
    for (int i = 0; i < cam.N; ++i) inl[i] = (xo_cell_err(&co, &pose, i, &cam) < cam.thr) ? 1 : 0;     /* as xo_refine */
    xo_normal_eq(&co, inl, &pose, &cam, out28);
    free(inl);
    return 0;
}
