/*
 * xl_dsac_math.h — the lane-local arithmetic of the DSAC* pose solver, written once.
 *
 * Everything one GPU lane (or one iteration of a CPU loop) computes on its own is here: the deterministic
 * transcendentals, the counter-based RNG, the rank plane and selection of the masked solver's compact sampler
 * (mask_rank_plane, mask_select), the camera record and the pixel centre of a cell (cam_make, cell_px), projection,
 * cell error and the soft-inlier sigmoid, the Ferrari quartic, P3P with its Newton polish and 4th-point selection, the
 * pieces of the Levenberg-Marquardt refinement (the per-cell normal equations, plain and weighted, the 6x6 Cholesky step,
 * the step-size stop and its constants, the not-NaN test of the result), the pose forms (12 doubles, float 4x4
 * cam->world), and the backward pass's Rodrigues maps, residual rows, pseudo-inverse and pose loss.  Consumers:
 *
 *   crossloc_amd/csrc/xl_dsac.hip   the product: HIP kernels (staging, ballots, wave / block reductions, the LM state machine)
 *   xl_dsac_quality_math.h, xl_dsac_refine_math.h and the RGB-D headers, which add their own passes' arithmetic on top
 *   oracle/dsac_oracle.c, tests/dsac_masked_ref.c and the other CPU restatements: test infrastructure, the same
 *                                   orchestration restated serially in C99 for gcc
 *
 * The dependency runs from the restatements to the headers only; nothing in the product path includes the oracle.
 *
 * Language: the common subset of C99 and HIP C++ (structs, pointers for out-parameters; no references, templates or
 * member functions).  hipcc includes it inside the consumer's namespace after <hip/hip_runtime.h>, <stdint.h> and
 * <string.h>; gcc gets the system headers from here.
 *
 * Arithmetic contract: only + - * / sqrt floor fabs and comparisons, compiled with -ffp-contract=off on both sides, so
 * gcc and hipcc produce identical bits from the identical sequence of IEEE operations.  Expression order and rounding
 * points are part of the interface: tests/test_oracle_dsac_pin.py pins the bits, tests/indep_dsac.py (an independent
 * implementation) guards the formulas themselves.  Reference line numbers are relative to the reference project's
 * dsacstar/ directory.
 */
#ifndef XL_DSAC_MATH_H
#define XL_DSAC_MATH_H

#if defined(__HIPCC__)
#define XL_MATH_FN __host__ __device__ __forceinline__
#define XL_MATH_CALL_FN __host__ __device__            /* inlining left to the compiler, as these always were */
#define XL_MATH_UNROLL _Pragma("unroll")
#define XL_MATH_NO_UNROLL _Pragma("unroll 1")
#else
#include <math.h>
#include <stdbool.h>
#include <stdint.h>
#include <string.h>
#define XL_MATH_FN static inline
#define XL_MATH_CALL_FN static
#define XL_MATH_UNROLL
#define XL_MATH_NO_UNROLL
#endif

#define XLM_PROB_THRESH 0.001          /* dsacstar_derivative.h:36 */
#define XLM_EPS 0.00000001             /* dsacstar_util.h:45 */
#define XLM_MAX_LOSS 10000000.0        /* dsacstar_loss.h:35 */
#define XLM_PI_REF 3.1415926           /* dsacstar_util.h:46 (calcAngularDistance) */
#define XLM_CV_PI 3.1415926535897932384626433832795
#define XLM_DBL_EPS 2.2204460492503131e-16
#define XLM_LM_MAX_ITER 20             /* cv::solvePnP ITERATIVE term criteria: iteration cap of every LM loop here ... */
#define XLM_FLT_EPS 1.1920928955078125e-07     /* ... and its epsilon (FLT_EPSILON), see lm_step_small */

typedef struct { double R[9]; double t[3]; } Pose;                   /* world -> camera */
typedef struct { double f, cx, cy; float thr, alpha, maxReproj; int sub, Ho, Wo, N; } Cam;
typedef struct { double x, y, z; } V3;
typedef struct { V3 e1, e2, e3; } Frame;
typedef struct { double Rc2w[9]; double C[3]; double R2[9]; double t2[3]; } Gt;   /* ground truth, both forms */

/* the one constructor of Cam.  The intrinsics arrive as the entry points' floats (widened exactly; a kernel passes
 * focals ? focals[b] : focal) or as the unit-test hooks' doubles */
XL_MATH_FN Cam cam_make(int Ho, int Wo, float thr, double f, double cx, double cy, float alpha, float maxReproj, int sub)
{
    Cam cam;
    cam.f = f; cam.cx = cx; cam.cy = cy;
    cam.thr = thr; cam.alpha = alpha; cam.maxReproj = maxReproj;
    cam.sub = sub; cam.Ho = Ho; cam.Wo = Wo; cam.N = Ho * Wo;
    return cam;
}

/* pixel centre of column (or row) i of the cell grid (createSampling, dsacstar_util.h:70-72) */
XL_MATH_FN float cell_px(const Cam *cam, int i) { return (float)(i * cam->sub + cam->sub / 2); }

/* ------------------------------------------------------------------------------ deterministic math */

XL_MATH_FN double bits_f64(uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)b);
#else
    double d; memcpy(&d, &b, 8); return d;
#endif
}

/* 2^k for k in [-1022, 1023] built from the exponent field (exact) */
XL_MATH_FN double pow2i(int k)
{
    return bits_f64((uint64_t)((long long)(k + 1023) << 52));
}

/* exp(x): k = floor(x/ln2 + 1/2), r = x - k ln2 (two-constant Cody-Waite), Taylor degree 14 */
XL_MATH_FN double det_exp(double x)
{
    if (x != x) return x;
    if (x > 709.0) return bits_f64(0x7ff0000000000000ULL);
    if (x < -708.0) return 0.0;
    const double INV_LN2 = 0x1.71547652b82fep+0;
    const double LN2_HI = 0x1.62e42f8000000p-1;
    const double LN2_LO = 0x1.be8e7bcd5e4f2p-27;
    double kf = floor(x * INV_LN2 + 0.5);
    double r = (x - kf * LN2_HI) - kf * LN2_LO;
    double p = 1.0 / 87178291200.0;              /* 1/14! */
    p = p * r + 1.0 / 6227020800.0;              /* 1/13! */
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * pow2i((int)kf);
}

/* sin and cos: k = floor(x*2/pi + 1/2), r = x - k*pi/2, Taylor degree 17 / 18 on [-pi/4, pi/4] */
XL_MATH_FN void det_sincos(double x, double *s, double *c)
{
    const double TWO_OVER_PI = 0x1.45f306dc9c883p-1;
    const double PIO2_HI = 0x1.921fb50000000p+0;
    const double PIO2_LO = 0x1.110b4611a6263p-26;
    double kf = floor(x * TWO_OVER_PI + 0.5);
    double r = (x - kf * PIO2_HI) - kf * PIO2_LO;
    double r2 = r * r;
    double ps = -1.0 / 355687428096000.0;        /* -1/17! */
    ps = ps * r2 + 1.0 / 1307674368000.0;        /* 1/15! */
    ps = ps * r2 - 1.0 / 6227020800.0;
    ps = ps * r2 + 1.0 / 39916800.0;
    ps = ps * r2 - 1.0 / 362880.0;
    ps = ps * r2 + 1.0 / 5040.0;
    ps = ps * r2 - 1.0 / 120.0;
    ps = ps * r2 + 1.0 / 6.0;
    double sr = r - r * r2 * ps;
    double pc = -1.0 / 6402373705728000.0;       /* -1/18! */
    pc = pc * r2 + 1.0 / 20922789888000.0;       /* 1/16! */
    pc = pc * r2 - 1.0 / 87178291200.0;
    pc = pc * r2 + 1.0 / 479001600.0;
    pc = pc * r2 - 1.0 / 3628800.0;
    pc = pc * r2 + 1.0 / 40320.0;
    pc = pc * r2 - 1.0 / 720.0;
    pc = pc * r2 + 1.0 / 24.0;
    double cr = 1.0 - r2 * (0.5 - r2 * pc);
    double q = kf - 4.0 * floor(kf * 0.25);      /* quadrant: k mod 4 (kf may be negative) */
    int qi = (int)q;
    if (qi == 0) { *s = sr; *c = cr; }
    else if (qi == 1) { *s = cr; *c = -sr; }
    else if (qi == 2) { *s = -sr; *c = -cr; }
    else { *s = -cr; *c = sr; }
}

/* ------------------------------------------------------------------------------ counter-based RNG */

XL_MATH_FN uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

/* state for (seed, image, hypothesis, try): the image part is the same for every try, so it is hashed once */
XL_MATH_FN uint64_t image_key(uint64_t seed, uint64_t image)
{
    return mix64(seed + 0x9e3779b97f4a7c15ULL * (image + 1));
}

XL_MATH_FN uint64_t try_state(uint64_t imageKey, uint32_t hyp, uint32_t t)
{
    return mix64(imageKey ^ (((uint64_t)hyp << 32) | (uint64_t)t));
}

/* irand(0, n) of thread_rand.cpp:68-71 semantics (uniform in [0, n)), multiply-shift; draw j of a try */
XL_MATH_FN int draw(uint64_t state, int j, int n)
{
    uint64_t r = mix64(state + 0x9e3779b97f4a7c15ULL * (uint64_t)(j + 1));
    uint32_t hi = (uint32_t)(r >> 32);
    return (int)(((uint64_t)hi * (uint64_t)(uint32_t)n) >> 32);
}

/* ------------------------------------------------------------------------------ compact sampler of the masked solver */

/* The validity mask as a bit plane (bit i & 31 of word i >> 5 <-> cell i, bits past the last cell zero) and its rank plane:
 * rank[w] = usable cells in words 0 .. w-1, for w = 0 .. nWords, so rank[nWords] = nUsable.  The kernel builds the plane with a
 * wave-level scan (xl_dsac.hip: build_rank_plane); this serial statement is the restatements'. */
XL_MATH_FN void mask_rank_plane(const uint32_t *words, int nWords, uint32_t *rank)
{
    uint32_t acc = 0;
    for (int w = 0; w < nWords; ++w) { rank[w] = acc; acc += (uint32_t)__builtin_popcount(words[w]); }
    rank[nWords] = acc;
}

/* cell index of the usable cell of rank k in row-major order, 0 <= k < rank[nWords]: binary search for the word w with
 * rank[w] <= k < rank[w + 1] (at most 9 steps at 16384 cells), then the set bit of rank k - rank[w] within it by popcount
 * halving.  Integers only. */
XL_MATH_FN int mask_select(const uint32_t *words, const uint32_t *rank, int nWords, int k)
{
    int lo = 0, hi = nWords;                               /* rank[lo] <= k < rank[hi] */
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rank[mid] <= (uint32_t)k) lo = mid; else hi = mid;
    }
    uint32_t v = words[lo];
    int r = k - (int)rank[lo], pos = 0;
    XL_MATH_UNROLL
    for (int width = 16; width >= 1; width >>= 1) {
        const int c = __builtin_popcount(v & ((1u << width) - 1u));
        if (r >= c) { r -= c; v >>= width; pos += width; }
    }
    return (lo << 5) + pos;
}

/* the four cells of a compact try: draw j is a rank in [0, nUsable), independent and with replacement */
XL_MATH_FN void compact_try_cells(uint64_t st, const uint32_t *words, const uint32_t *rank, int nWords, int *cells)
{
    const int nUsable = (int)rank[nWords];
    XL_MATH_UNROLL
    for (int j = 0; j < 4; ++j) cells[j] = mask_select(words, rank, nWords, draw(st, j, nUsable));
}

/* ------------------------------------------------------------------------------ projection + cell error */

/* cv::projectPoints restated: float pixel, no cheirality test (dsacstar_util.h:199-205, 395-401) */
XL_MATH_FN void project(const Pose *p, double X, double Y, double Z, const Cam *cam, float *u, float *v)
{
    double xc = p->R[0] * X + p->R[1] * Y + p->R[2] * Z + p->t[0];
    double yc = p->R[3] * X + p->R[4] * Y + p->R[5] * Z + p->t[1];
    double zc = p->R[6] * X + p->R[7] * Y + p->R[8] * Z + p->t[2];
    double z = (zc != 0.0) ? 1.0 / zc : 1.0;
    double x = xc * z, y = yc * z;
    *u = (float)(x * cam->f + cam->cx);
    *v = (float)(y * cam->f + cam->cy);
}

/* reprojection error of the scene coordinate (X, Y, Z) of cell (y, x) against the cell's pixel centre, clamped:
 * std::min(err, maxReproj) (dsacstar_util.h:438-443) */
XL_MATH_FN float cell_err(const Pose *p, double X, double Y, double Z, int y, int x, const Cam *cam)
{
    float u, v;
    project(p, X, Y, Z, cam, &u, &v);
    float dx = cell_px(cam, x) - u, dy = cell_px(cam, y) - v;
    double n = sqrt((double)dx * (double)dx + (double)dy * (double)dy);
    float a = (float)n;
    return (cam->maxReproj < a) ? cam->maxReproj : a;
}

/* soft-inlier sigmoid of a cell with clamped error e (getHypScores, dsacstar_util.h:316-343; beta = 5 / thr): the score
 * term of the cell is 1.0 - st, the backward pass's derivative uses st * (1.0 - st) */
XL_MATH_FN double soft_inlier_st(float e, float thr, float beta)
{
    float stf = beta * (e - thr);
    return 1.0 / (1.0 + det_exp(-(double)stf));
}

/* ------------------------------------------------------------------------------ quartic (Ferrari) */

/* a positive real root of g(z) = z^3 + c2 z^2 + c1 z + c0 with g(0) <= 0: Newton safeguarded by the bracket [lo, hi]
 * (g(lo) <= 0 < g(hi), hi starts at the Cauchy bound); bisect when Newton leaves it */
XL_MATH_FN double cubic_pos_root(double c2, double c1, double c0)
{
    double m = fabs(c2);
    if (fabs(c1) > m) m = fabs(c1);
    if (fabs(c0) > m) m = fabs(c0);
    double lo = 0.0, hi = 1.0 + m;
    double z = hi;
    for (int it = 0; it < 128; ++it) {
        double g = ((z + c2) * z + c1) * z + c0;
        double dg = (3.0 * z + 2.0 * c2) * z + c1;
        if (g > 0.0) hi = z; else lo = z;
        if (g == 0.0) break;
        double zn = z - g / dg;
        if (!(zn > lo && zn < hi)) zn = 0.5 * (lo + hi);
        if (zn == z || !(hi > lo)) break;
        z = zn;
    }
    return z;
}

/* real roots of y^2 + b y + c (numerically stable pair) */
XL_MATH_FN bool quadratic(double b, double c, double *r0, double *r1)
{
    double disc = b * b - 4.0 * c;
    if (!(disc >= 0.0)) return false;
    double sq = sqrt(disc);
    double q = (b >= 0.0) ? -0.5 * (b + sq) : -0.5 * (b - sq);
    if (q != 0.0) { *r0 = q; *r1 = c / q; }
    else { *r0 = 0.0; *r1 = 0.0; }
    return true;
}

/* real roots of A4 x^4 + A3 x^3 + A2 x^2 + A1 x + A0, A4 != 0: four fixed slots, bit i of the result set when slot i
 * holds a root (each quadratic factor fills a pair) */
XL_MATH_FN unsigned quartic(double A4, double A3, double A2, double A1, double A0,
                            double *x0, double *x1, double *x2, double *x3)
{
    double a = A3 / A4, b = A2 / A4, c = A1 / A4, d = A0 / A4;
    double a2 = a * a;
    double p = b - 0.375 * a2;
    double q = c - 0.5 * a * b + 0.125 * a2 * a;
    double r = d - 0.25 * a * c + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2;
    double shift = -0.25 * a;
    unsigned mask = 0;
    *x0 = *x1 = *x2 = *x3 = 0.0;
    double z0 = cubic_pos_root(2.0 * p, p * p - 4.0 * r, -(q * q));
    if (z0 > 0.0) {
        double s = sqrt(z0);
        double h = 0.5 * (p + z0);
        double g = 0.5 * q / s;
        double r0, r1;
        if (quadratic(s, h - g, &r0, &r1)) { *x0 = r0 + shift; *x1 = r1 + shift; mask |= 3u; }
        if (quadratic(-s, h + g, &r0, &r1)) { *x2 = r0 + shift; *x3 = r1 + shift; mask |= 12u; }
    } else {
        /* biquadratic: y^4 + p y^2 + r */
        double w0, w1;
        if (quadratic(p, r, &w0, &w1)) {
            if (w0 >= 0.0) { double y = sqrt(w0); *x0 = y + shift; *x1 = -y + shift; mask |= 3u; }
            if (w1 >= 0.0) { double y = sqrt(w1); *x2 = y + shift; *x3 = -y + shift; mask |= 12u; }
        }
    }
    return mask;
}

/* ------------------------------------------------------------------------------ P3P + 4th point */

XL_MATH_FN V3 cross3(V3 a, V3 b)
{
    V3 o = { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x };
    return o;
}

/* orthonormal frame of triangle (A,B,C): e1 along AB, e3 normal, e2 = e3 x e1; false if degenerate */
XL_MATH_FN bool frame_of(V3 A, V3 B, V3 C, Frame *F)
{
    V3 ab = { B.x - A.x, B.y - A.y, B.z - A.z };
    V3 ac = { C.x - A.x, C.y - A.y, C.z - A.z };
    double n1 = sqrt(ab.x * ab.x + ab.y * ab.y + ab.z * ab.z);
    if (!(n1 > 0.0)) return false;
    V3 e1 = { ab.x / n1, ab.y / n1, ab.z / n1 };
    F->e1 = e1;
    V3 nn = cross3(ab, ac);
    double n3 = sqrt(nn.x * nn.x + nn.y * nn.y + nn.z * nn.z);
    if (!(n3 > 0.0)) return false;
    V3 e3 = { nn.x / n3, nn.y / n3, nn.z / n3 };
    F->e3 = e3;
    F->e2 = cross3(F->e3, F->e1);
    return true;
}

XL_MATH_FN V3 bearing(double u, double v, const Cam *cam)
{
    double mx = (u - cam->cx) / cam->f, my = (v - cam->cy) / cam->f;
    double nrm = sqrt(mx * mx + my * my + 1.0);
    V3 o = { mx / nrm, my / nrm, 1.0 / nrm };
    return o;
}

/* one root of the quartic -> distances (two Newton steps on the law-of-cosines system), rigid alignment through the two
 * triangle frames, squared pixel error of the 4th point (double, no z test); false if the root is rejected */
XL_MATH_FN bool p3p_candidate(double v, double pq, double ca, double cb, double cg, double a2, double b2, double c2,
                              V3 f0, V3 f1, V3 f2, V3 P0, V3 P1, V3 P2, V3 P3,
                              double u3, double v3, const Frame *E, const Cam *cam, Pose *cand, double *err)
{
    if (!(v > 0.0)) return false;
    double den = cg - v * ca;
    if (!(den != 0.0)) return false;
    double u = ((pq - 1.0) * v * v - 2.0 * pq * cb * v + 1.0 + pq) / (2.0 * den);
    if (!(u > 0.0)) return false;
    double w = 1.0 + v * v - 2.0 * v * cb;
    if (!(w > 0.0)) return false;
    double s1 = sqrt(b2 / w), s2 = u * s1, s3 = v * s1;
    for (int it = 0; it < 2; ++it) {
        double F1 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2;
        double F2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - b2;
        double F3 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2;
        double j12 = 2.0 * s2 - 2.0 * s3 * ca, j13 = 2.0 * s3 - 2.0 * s2 * ca;
        double j21 = 2.0 * s1 - 2.0 * s3 * cb, j23 = 2.0 * s3 - 2.0 * s1 * cb;
        double j31 = 2.0 * s1 - 2.0 * s2 * cg, j32 = 2.0 * s2 - 2.0 * s1 * cg;
        /* J = [[0,j12,j13],[j21,0,j23],[j31,j32,0]] */
        double det = j12 * j23 * j31 + j13 * j21 * j32;
        if (!(det != 0.0)) break;
        double dx1 = (F1 * (-(j23 * j32)) - j12 * (-(j23 * F3)) + j13 * (F2 * j32)) / det;
        double dx2 = (-(F1 * (-(j23 * j31))) + j13 * (j21 * F3 - F2 * j31)) / det;
        double dx3 = (-(j12 * (j21 * F3 - F2 * j31)) + F1 * (j21 * j32)) / det;
        s1 -= dx1; s2 -= dx2; s3 -= dx3;
    }
    if (!(s1 > 0.0) || !(s2 > 0.0) || !(s3 > 0.0)) return false;
    V3 C0 = { s1 * f0.x, s1 * f0.y, s1 * f0.z };
    V3 C1 = { s2 * f1.x, s2 * f1.y, s2 * f1.z };
    V3 C2 = { s3 * f2.x, s3 * f2.y, s3 * f2.z };
    Frame D;
    if (!frame_of(C0, C1, C2, &D)) return false;
    /* R[i][j] = d1[i] e1[j] + d2[i] e2[j] + d3[i] e3[j] */
    cand->R[0] = D.e1.x * E->e1.x + D.e2.x * E->e2.x + D.e3.x * E->e3.x;
    cand->R[1] = D.e1.x * E->e1.y + D.e2.x * E->e2.y + D.e3.x * E->e3.y;
    cand->R[2] = D.e1.x * E->e1.z + D.e2.x * E->e2.z + D.e3.x * E->e3.z;
    cand->R[3] = D.e1.y * E->e1.x + D.e2.y * E->e2.x + D.e3.y * E->e3.x;
    cand->R[4] = D.e1.y * E->e1.y + D.e2.y * E->e2.y + D.e3.y * E->e3.y;
    cand->R[5] = D.e1.y * E->e1.z + D.e2.y * E->e2.z + D.e3.y * E->e3.z;
    cand->R[6] = D.e1.z * E->e1.x + D.e2.z * E->e2.x + D.e3.z * E->e3.x;
    cand->R[7] = D.e1.z * E->e1.y + D.e2.z * E->e2.y + D.e3.z * E->e3.y;
    cand->R[8] = D.e1.z * E->e1.z + D.e2.z * E->e2.z + D.e3.z * E->e3.z;
    /* t = centroid_c - R centroid_w */
    double pwx = (P0.x + P1.x + P2.x) / 3.0, pwy = (P0.y + P1.y + P2.y) / 3.0, pwz = (P0.z + P1.z + P2.z) / 3.0;
    double pcx = (C0.x + C1.x + C2.x) / 3.0, pcy = (C0.y + C1.y + C2.y) / 3.0, pcz = (C0.z + C1.z + C2.z) / 3.0;
    cand->t[0] = pcx - (cand->R[0] * pwx + cand->R[1] * pwy + cand->R[2] * pwz);
    cand->t[1] = pcy - (cand->R[3] * pwx + cand->R[4] * pwy + cand->R[5] * pwz);
    cand->t[2] = pcz - (cand->R[6] * pwx + cand->R[7] * pwy + cand->R[8] * pwz);
    double xc = cand->R[0] * P3.x + cand->R[1] * P3.y + cand->R[2] * P3.z + cand->t[0];
    double yc = cand->R[3] * P3.x + cand->R[4] * P3.y + cand->R[5] * P3.z + cand->t[1];
    double zc = cand->R[6] * P3.x + cand->R[7] * P3.y + cand->R[8] * P3.z + cand->t[2];
    double up = cam->cx + cam->f * xc / zc, vp = cam->cy + cam->f * yc / zc;
    *err = (up - u3) * (up - u3) + (vp - v3) * (vp - v3);
    return true;
}

XL_MATH_FN void pose_identity(Pose *p)
{
    p->R[0] = 1.0; p->R[1] = 0.0; p->R[2] = 0.0;
    p->R[3] = 0.0; p->R[4] = 1.0; p->R[5] = 0.0;
    p->R[6] = 0.0; p->R[7] = 0.0; p->R[8] = 1.0;
    p->t[0] = 0.0; p->t[1] = 0.0; p->t[2] = 0.0;
}

/* a pose as 12 doubles: R row-major, then t */
XL_MATH_FN void pose_load12(const double *src, Pose *p)
{
    XL_MATH_UNROLL
    for (int i = 0; i < 9; ++i) p->R[i] = src[i];
    XL_MATH_UNROLL
    for (int i = 0; i < 3; ++i) p->t[i] = src[9 + i];
}

XL_MATH_FN void pose_store12(const Pose *p, double *dst)
{
    XL_MATH_UNROLL
    for (int i = 0; i < 9; ++i) dst[i] = p->R[i];
    XL_MATH_UNROLL
    for (int i = 0; i < 3; ++i) dst[9 + i] = p->t[i];
}

/* cv::solvePnP(SOLVEPNP_P3P) call-site contract (dsacstar_util.h:185-193): object points P0..P2 and pixels uv[0..2]
 * solve (law-of-cosines quartic, Grunert form of the Gao et al. system), the candidate with the smallest error on the
 * 4th point wins.  Returns true and the world -> camera pose on success. */
XL_MATH_CALL_FN bool p3p(V3 P0, V3 P1, V3 P2, V3 P3, const double uv[4][2], const Cam *cam, Pose *out)
{
    V3 f0 = bearing(uv[0][0], uv[0][1], cam);
    V3 f1 = bearing(uv[1][0], uv[1][1], cam);
    V3 f2 = bearing(uv[2][0], uv[2][1], cam);
    double ca = f1.x * f2.x + f1.y * f2.y + f1.z * f2.z;
    double cb = f0.x * f2.x + f0.y * f2.y + f0.z * f2.z;
    double cg = f0.x * f1.x + f0.y * f1.y + f0.z * f1.z;
    double d0, d1, d2;
    d0 = P1.x - P2.x; d1 = P1.y - P2.y; d2 = P1.z - P2.z;
    double a2 = d0 * d0 + d1 * d1 + d2 * d2;
    d0 = P0.x - P2.x; d1 = P0.y - P2.y; d2 = P0.z - P2.z;
    double b2 = d0 * d0 + d1 * d1 + d2 * d2;
    d0 = P0.x - P1.x; d1 = P0.y - P1.y; d2 = P0.z - P1.z;
    double c2 = d0 * d0 + d1 * d1 + d2 * d2;
    if (!(a2 > 0.0) || !(b2 > 0.0) || !(c2 > 0.0)) return false;
    Frame E;
    if (!frame_of(P0, P1, P2, &E)) return false;

    double pq = (a2 - c2) / b2, qq = (a2 + c2) / b2;
    double c2b = c2 / b2, a2b = a2 / b2;
    double A4 = (pq - 1.0) * (pq - 1.0) - 4.0 * c2b * ca * ca;
    double A3 = 4.0 * (pq * (1.0 - pq) * cb - (1.0 - qq) * ca * cg + 2.0 * c2b * ca * ca * cb);
    double A2 = 2.0 * (pq * pq - 1.0 + 2.0 * pq * pq * cb * cb + 2.0 * ((b2 - c2) / b2) * ca * ca
                       - 4.0 * qq * ca * cb * cg + 2.0 * ((b2 - a2) / b2) * cg * cg);
    double A1 = 4.0 * (-pq * (1.0 + pq) * cb + 2.0 * a2b * cg * cg * cb - (1.0 - qq) * ca * cg);
    double A0 = (1.0 + pq) * (1.0 + pq) - 4.0 * a2b * cg * cg;
    if (!(A4 != 0.0) || A4 != A4) return false;

    double x0, x1, x2, x3;
    unsigned mask = quartic(A4, A3, A2, A1, A0, &x0, &x1, &x2, &x3);
    bool found = false;
    double best = 0.0;
    XL_MATH_NO_UNROLL
    for (int ri = 0; ri < 4; ++ri) {
        if (!((mask >> ri) & 1u)) continue;
        double v = (ri == 0) ? x0 : (ri == 1) ? x1 : (ri == 2) ? x2 : x3;
        Pose cand;
        double e;
        if (!p3p_candidate(v, pq, ca, cb, cg, a2, b2, c2, f0, f1, f2, P0, P1, P2, P3,
                           uv[3][0], uv[3][1], &E, cam, &cand, &e)) continue;
        if (!found || e < best) { best = e; *out = cand; found = true; }
    }
    return found;
}

/* ------------------------------------------------------------------------------ LM pieces */

/* pose2trans: the float 4x4 cam->world matrix (row-major) of a world -> camera pose, the inverse rigid transform as the
 * solver's write step forms it */
XL_MATH_FN void pose_to_c2w16(const Pose *p, float *o)
{
    XL_MATH_UNROLL
    for (int i = 0; i < 3; ++i) {
        XL_MATH_UNROLL
        for (int j = 0; j < 3; ++j) o[4 * i + j] = (float)p->R[3 * j + i];
        o[4 * i + 3] = (float)(-(p->R[i] * p->t[0] + p->R[3 + i] * p->t[1] + p->R[6 + i] * p->t[2]));
    }
    o[12] = 0.0f; o[13] = 0.0f; o[14] = 0.0f; o[15] = 1.0f;
}

/* no entry of the pose is NaN: the test the solver makes on an LM result (x == x; an infinite entry passes.  The
 * stand-alone passes ask for finite entries instead: quality_pose_finite) */
XL_MATH_FN bool pose_not_nan(const Pose *p)
{
    bool ok = true;
    XL_MATH_UNROLL
    for (int i = 0; i < 9; ++i) if (!(p->R[i] == p->R[i])) ok = false;
    XL_MATH_UNROLL
    for (int i = 0; i < 3; ++i) if (!(p->t[i] == p->t[i])) ok = false;
    return ok;
}

/* the per-cell PnP rows at pose p for the cell (y, x) with scene coordinate (X, Y, Z): the residual (ru, rv) of the double
 * projection against the pixel centre and its Jacobian rows Ju, Jv w.r.t. the increment (w, d) of apply_step.  The one
 * statement of these formulas: the solver's refinement, the pose-quality pass, the weighted refinement and their CPU
 * restatements all accumulate it through one of the two functions below; the only other expansion is the solver kernel's
 * normal_eq_thread (xl_dsac.hip), for the reason given there.
 * A macro over the names p, X, Y, Z, y, x, cam of the expanding function, not a function: with the rows behind a
 * force-inlined function (out-pointers or a struct by value alike) hipcc schedules the cell loops differently at equal
 * register figures - measured on MI355X against the hand-written loops, same session: the weighted refinement alone
 * 0.548 against 0.525 ms per 95 frames (+4 %), the solver's single-frame call 0.2564 against 0.2541 ms (+0.8 %).  As text
 * the consumers compile to the instructions of the hand-written loops (tools/kernel_asm_diff.py). */
#define XL_PNP_CELL_ROWS \
    double Ju[6], Jv[6], ru, rv; \
    { \
        double qx = p->R[0] * X + p->R[1] * Y + p->R[2] * Z; \
        double qy = p->R[3] * X + p->R[4] * Y + p->R[5] * Z; \
        double qz = p->R[6] * X + p->R[7] * Y + p->R[8] * Z; \
        double xc = qx + p->t[0], yc = qy + p->t[1], zc = qz + p->t[2]; \
        double z = (zc != 0.0) ? 1.0 / zc : 1.0; \
        double xn = xc * z, yn = yc * z; \
        ru = (xn * cam->f + cam->cx) - (double)cell_px(cam, x); \
        rv = (yn * cam->f + cam->cy) - (double)cell_px(cam, y); \
        double fa = cam->f * z;             /* du/dXc = dv/dYc */ \
        double fc = -(fa * xn);             /* du/dZc */ \
        double fd = -(fa * yn);             /* dv/dZc */ \
        Ju[0] = fc * qy;            Ju[1] = fa * qz - fc * qx;  Ju[2] = -(fa * qy); \
        Ju[3] = fa;                 Ju[4] = 0.0;                Ju[5] = fc; \
        Jv[0] = fd * qy - fa * qz;  Jv[1] = -(fd * qx);         Jv[2] = fa * qx; \
        Jv[3] = 0.0;                Jv[4] = fa;                 Jv[5] = fd; \
    }

/* what the cell adds to the 28 normal-equation sums: a[0..20] += upper triangle of Ju Ju^T + Jv Jv^T (row-major),
 * a[21..26] += J^T r, a[27] += ru^2 + rv^2 */
XL_MATH_FN void pnp_cell_normal_eq(const Pose *p, double X, double Y, double Z, int y, int x, const Cam *cam, double *a)
{
    XL_PNP_CELL_ROWS
    int k = 0;
    XL_MATH_UNROLL
    for (int r = 0; r < 6; ++r)
        XL_MATH_UNROLL
        for (int c = r; c < 6; ++c) { a[k] += Ju[r] * Ju[c] + Jv[r] * Jv[c]; ++k; }
    XL_MATH_UNROLL
    for (int r = 0; r < 6; ++r) a[21 + r] += Ju[r] * ru + Jv[r] * rv;
    a[27] += ru * ru + rv * rv;
}

/* the same with the cell's contribution to each sum multiplied by w.  An accumulator of its own: the solver does not pay
 * for the multiplications, and since the PRODUCTS are multiplied, not the rows, w == 1.0 gives the unweighted bits */
XL_MATH_FN void pnp_cell_normal_eq_w(const Pose *p, double X, double Y, double Z, double w, int y, int x, const Cam *cam,
                                     double *a)
{
    XL_PNP_CELL_ROWS
    int k = 0;
    XL_MATH_UNROLL
    for (int r = 0; r < 6; ++r)
        XL_MATH_UNROLL
        for (int c = r; c < 6; ++c) { a[k] += w * (Ju[r] * Ju[c] + Jv[r] * Jv[c]); ++k; }
    XL_MATH_UNROLL
    for (int r = 0; r < 6; ++r) a[21 + r] += w * (Ju[r] * ru + Jv[r] * rv);
    a[27] += w * (ru * ru + rv * rv);
}

/* the step-size stop of every Levenberg-Marquardt loop here: |d|^2 < FLT_EPSILON^2 |param|^2 */
XL_MATH_FN bool lm_step_small(const double *d, const Pose *prev)
{
    double dn = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5];
    double pn = (3.0 - (prev->R[0] + prev->R[4] + prev->R[8]))
                + prev->t[0] * prev->t[0] + prev->t[1] * prev->t[1] + prev->t[2] * prev->t[2];
    return dn < XLM_FLT_EPS * XLM_FLT_EPS * pn;
}

/* solve (JtJ with diag*(1+lambda)) d = Jtr by Cholesky; false on breakdown */
XL_MATH_FN bool solve6(const double *ne, double lambda, double *d)
{
    double A[6][6];
    {
        int k = 0;
        XL_MATH_UNROLL
        for (int r = 0; r < 6; ++r)
            XL_MATH_UNROLL
            for (int c = r; c < 6; ++c) { A[r][c] = ne[k]; A[c][r] = ne[k]; ++k; }
    }
    XL_MATH_UNROLL
    for (int r = 0; r < 6; ++r) A[r][r] = A[r][r] * (1.0 + lambda);
    double L[6][6];
    XL_MATH_UNROLL
    for (int i = 0; i < 6; ++i)
        XL_MATH_UNROLL
        for (int j = 0; j < 6; ++j) L[i][j] = 0.0;
    bool ok = true;
    XL_MATH_UNROLL
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        XL_MATH_UNROLL
        for (int m = 0; m < j; ++m) s -= L[j][m] * L[j][m];
        if (!(s > 0.0)) ok = false;
        double ljj = sqrt(s);
        L[j][j] = ljj;
        XL_MATH_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            XL_MATH_UNROLL
            for (int m = 0; m < j; ++m) v -= L[i][m] * L[j][m];
            L[i][j] = v / ljj;
        }
    }
    if (!ok) return false;
    double yv[6];
    XL_MATH_UNROLL
    for (int i = 0; i < 6; ++i) {
        double v = ne[21 + i];
        XL_MATH_UNROLL
        for (int m = 0; m < i; ++m) v -= L[i][m] * yv[m];
        yv[i] = v / L[i][i];
    }
    XL_MATH_UNROLL
    for (int i = 5; i >= 0; --i) {
        double v = yv[i];
        XL_MATH_UNROLL
        for (int m = i + 1; m < 6; ++m) v -= L[m][i] * d[m];
        d[i] = v / L[i][i];
    }
    XL_MATH_UNROLL
    for (int i = 0; i < 6; ++i)
        if (!(d[i] == d[i]) || fabs(d[i]) > 1.0e300) ok = false;
    return ok;
}

/* param = prev (-) d : R = Exp(-d_w) R_prev, t = t_prev - d_t */
XL_MATH_FN void apply_step(const Pose *prev, const double *d, Pose *out)
{
    double wx = -d[0], wy = -d[1], wz = -d[2];
    double th2 = wx * wx + wy * wy + wz * wz;
    double th = sqrt(th2);
    double E[9];
    if (!(th > 1.0e-300)) {
        E[0] = 1.0; E[1] = -wz; E[2] = wy;
        E[3] = wz;  E[4] = 1.0; E[5] = -wx;
        E[6] = -wy; E[7] = wx;  E[8] = 1.0;
    } else {
        double s, c;
        det_sincos(th, &s, &c);
        double kx = wx / th, ky = wy / th, kz = wz / th;
        double c1 = 1.0 - c;
        E[0] = c + c1 * kx * kx;      E[1] = c1 * kx * ky - s * kz; E[2] = c1 * kx * kz + s * ky;
        E[3] = c1 * kx * ky + s * kz; E[4] = c + c1 * ky * ky;      E[5] = c1 * ky * kz - s * kx;
        E[6] = c1 * kx * kz - s * ky; E[7] = c1 * ky * kz + s * kx; E[8] = c + c1 * kz * kz;
    }
    XL_MATH_UNROLL
    for (int i = 0; i < 3; ++i)
        XL_MATH_UNROLL
        for (int j = 0; j < 3; ++j)
            out->R[3 * i + j] = E[3 * i] * prev->R[j] + E[3 * i + 1] * prev->R[3 + j] + E[3 * i + 2] * prev->R[6 + j];
    out->t[0] = prev->t[0] - d[3];
    out->t[1] = prev->t[1] - d[4];
    out->t[2] = prev->t[2] - d[5];
}

/* CvLevMarq damping 10^lg for lg in [-16, 16]; decimal literals, identical constants on host and device */
XL_MATH_FN double lambda_of(int lg)
{
    switch (lg) {
        case -16: return 1e-16; case -15: return 1e-15; case -14: return 1e-14; case -13: return 1e-13;
        case -12: return 1e-12; case -11: return 1e-11; case -10: return 1e-10; case -9: return 1e-9;
        case -8: return 1e-8; case -7: return 1e-7; case -6: return 1e-6; case -5: return 1e-5;
        case -4: return 1e-4; case -3: return 1e-3; case -2: return 1e-2; case -1: return 1e-1;
        case 0: return 1e0; case 1: return 1e1; case 2: return 1e2; case 3: return 1e3; case 4: return 1e4;
        case 5: return 1e5; case 6: return 1e6; case 7: return 1e7; case 8: return 1e8; case 9: return 1e9;
        case 10: return 1e10; case 11: return 1e11; case 12: return 1e12; case 13: return 1e13;
        case 14: return 1e14; case 15: return 1e15; default: return 1e16;
    }
}

/* ============================================================================== backward_rgb */

/* atan2 from + - * / sqrt and det_sincos only: rational first guess (error < 5e-3), then Newton-like corrections
 * t += asin(sin(target - t)) with the asin series to 5th order (error after one step ~1e-17, two more for margin) */
XL_MATH_CALL_FN double det_atan2(double y, double x)
{
    if (x == 0.0 && y == 0.0) return 0.0;
    double n = sqrt(x * x + y * y);
    double cn = x / n, sn = y / n;
    double ax = fabs(x), ay = fabs(y);
    double t;
    if (ay <= ax) { double a = ay / ax; t = a / (1.0 + 0.28 * a * a); }
    else { double a = ax / ay; t = 1.5707963267948966 - a / (1.0 + 0.28 * a * a); }
    if (x < 0.0) t = 3.141592653589793 - t;
    if (y < 0.0) t = -t;
    for (int it = 0; it < 3; ++it) {
        double s, c;
        det_sincos(t, &s, &c);
        double d = sn * c - cn * s;
        double d2 = d * d;
        t = t + d * (1.0 + d2 * (1.0 / 6.0 + d2 * (3.0 / 40.0)));
    }
    return t;
}

XL_MATH_CALL_FN double det_acos(double v) { return det_atan2(sqrt((1.0 - v) * (1.0 + v)), v); }

/* cv::Rodrigues(matrix -> vector) for a rotation matrix; atan2(sin, cos) where OpenCV uses acos(cos) */
XL_MATH_CALL_FN void log_so3(const double *R, double *r)
{
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1.0) * 0.5;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    double theta = det_atan2(s, c);
    if (s < 1e-5) {
        if (c > 0.0) { r[0] = 0.0; r[1] = 0.0; r[2] = 0.0; return; }
        double t;
        t = (R[0] + 1.0) * 0.5; rx = sqrt(t > 0.0 ? t : 0.0);
        t = (R[4] + 1.0) * 0.5; ry = sqrt(t > 0.0 ? t : 0.0) * (R[1] < 0.0 ? -1.0 : 1.0);
        t = (R[8] + 1.0) * 0.5; rz = sqrt(t > 0.0 ? t : 0.0) * (R[2] < 0.0 ? -1.0 : 1.0);
        if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && ((R[5] > 0.0) != (ry * rz > 0.0))) rz = -rz;
        theta = theta / sqrt(rx * rx + ry * ry + rz * rz);
        r[0] = rx * theta; r[1] = ry * theta; r[2] = rz * theta;
        return;
    }
    double vth = (1.0 / (2.0 * s)) * theta;
    r[0] = rx * vth; r[1] = ry * vth; r[2] = rz * vth;
}

/* cv::Rodrigues(vector -> matrix) */
XL_MATH_CALL_FN void exp_so3(const double *r, double *R)
{
    double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (th < XLM_DBL_EPS) {
        for (int i = 0; i < 9; ++i) R[i] = 0.0;
        R[0] = 1.0; R[4] = 1.0; R[8] = 1.0;
        return;
    }
    double s, c;
    det_sincos(th, &s, &c);
    double c1 = 1.0 - c, ith = 1.0 / th;
    double kx = r[0] * ith, ky = r[1] * ith, kz = r[2] * ith;
    R[0] = c + c1 * kx * kx;      R[1] = c1 * kx * ky - s * kz; R[2] = c1 * kx * kz + s * ky;
    R[3] = c1 * kx * ky + s * kz; R[4] = c + c1 * ky * ky;      R[5] = c1 * ky * kz - s * kx;
    R[6] = c1 * kx * kz - s * ky; R[7] = c1 * ky * kz + s * kx; R[8] = c + c1 * kz * kz;
}

/* dR[(3a+b)*3 + c] = d R[a][b] / d r_c at rotation vector r (the transpose of OpenCV's 3x9 jacobian): the exact
 * derivative of R = cos t I + (1 - cos t) k k^T + sin t [k]x */
XL_MATH_CALL_FN void rodrigues_jac(const double *r, double *dR)
{
    double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    for (int i = 0; i < 27; ++i) dR[i] = 0.0;
    if (th < XLM_DBL_EPS) {
        /* generators: d/dr_x = [[0,0,0],[0,0,-1],[0,1,0]] etc. */
        dR[5 * 3 + 0] = -1.0; dR[7 * 3 + 0] = 1.0;
        dR[2 * 3 + 1] = 1.0;  dR[6 * 3 + 1] = -1.0;
        dR[1 * 3 + 2] = -1.0; dR[3 * 3 + 2] = 1.0;
        return;
    }
    double s, c;
    det_sincos(th, &s, &c);
    double c1 = 1.0 - c, ith = 1.0 / th;
    double k[3] = { r[0] * ith, r[1] * ith, r[2] * ith };
    for (int i = 0; i < 3; ++i) {
        double dk[3];
        for (int j = 0; j < 3; ++j) dk[j] = ((i == j ? 1.0 : 0.0) - k[i] * k[j]) * ith;
        double ski = s * k[i], cki = c * k[i];
        /* K = [k]x, dK = [dk]x */
        double K[9] = { 0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0 };
        double dK[9] = { 0.0, -dk[2], dk[1], dk[2], 0.0, -dk[0], -dk[1], dk[0], 0.0 };
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double v = ski * (k[a] * k[b]) + c1 * (dk[a] * k[b] + k[a] * dk[b]) + cki * K[3 * a + b] + s * dK[3 * a + b];
                if (a == b) v -= ski;
                dR[(3 * a + b) * 3 + i] = v;
            }
    }
}

/* Row of the residual Jacobian of one cell at pose p with rotation-vector derivative dR:
 * J6 = d max(|proj - pt|, EPS) / d (rvec, tvec), all-zero when that error exceeds maxReproj
 * (dsacstar_util.h:403-434, dsacstar.cpp:386-405).  Returns the (unclamped) error. */
XL_MATH_CALL_FN double resid_row(const Pose *p, const double *dR, double X, double Y, double Z, float px, float py,
                                 const Cam *cam, double *J6)
{
    double qx = p->R[0] * X + p->R[1] * Y + p->R[2] * Z;
    double qy = p->R[3] * X + p->R[4] * Y + p->R[5] * Z;
    double qz = p->R[6] * X + p->R[7] * Y + p->R[8] * Z;
    double xc = qx + p->t[0], yc = qy + p->t[1], zc = qz + p->t[2];
    double z = (zc != 0.0) ? 1.0 / zc : 1.0;
    double xn = xc * z, yn = yc * z;
    float uf = (float)(xn * cam->f + cam->cx), vf = (float)(yn * cam->f + cam->cy);
    float dxf = uf - px, dyf = vf - py;
    double err = sqrt((double)dxf * (double)dxf + (double)dyf * (double)dyf);
    if (err < XLM_EPS) err = XLM_EPS;
    XL_MATH_UNROLL
    for (int i = 0; i < 6; ++i) J6[i] = 0.0;
    if (err > (double)cam->maxReproj) return err;
    double nx = 1.0 / err * (double)dxf, ny = 1.0 / err * (double)dyf;
    double fa = cam->f * z;             /* du/dXc = dv/dYc */
    double fc = -(fa * xn);             /* du/dZc */
    double fd = -(fa * yn);             /* dv/dZc */
    XL_MATH_UNROLL
    for (int c = 0; c < 3; ++c) {
        double dX = dR[0 * 3 + c] * X + dR[1 * 3 + c] * Y + dR[2 * 3 + c] * Z;
        double dY = dR[3 * 3 + c] * X + dR[4 * 3 + c] * Y + dR[5 * 3 + c] * Z;
        double dZ = dR[6 * 3 + c] * X + dR[7 * 3 + c] * Y + dR[8 * 3 + c] * Z;
        double ju = fa * dX + fc * dZ, jv = fa * dY + fd * dZ;
        J6[c] = nx * ju + ny * jv;
    }
    J6[3] = nx * fa;
    J6[4] = ny * fa;
    J6[5] = nx * fc + ny * fd;
    return err;
}

/* dProjectdObj, dsacstar_derivative.h:51-106 (expression order kept) */
XL_MATH_CALL_FN void dproject_dobj(const Pose *p, double X, double Y, double Z, float ptx, float pty, const Cam *cam,
                                   double *out)
{
    out[0] = 0.0; out[1] = 0.0; out[2] = 0.0;
    double ox = p->R[0] * X + p->R[1] * Y + p->R[2] * Z + p->t[0];
    double oy = p->R[3] * X + p->R[4] * Y + p->R[5] * Z + p->t[1];
    double oz = p->R[6] * X + p->R[7] * Y + p->R[8] * Z + p->t[2];
    if (fabs(oz) < XLM_EPS) return;
    double px = cam->f * ox / oz + cam->cx;
    double py = cam->f * oy / oz + cam->cy;
    double ex = (double)ptx - px, ey = (double)pty - py;
    double err = sqrt(ex * ex + ey * ey);
    if (err > (double)cam->maxReproj) return;
    err += XLM_EPS;
    XL_MATH_UNROLL
    for (int k = 0; k < 3; ++k) {
        double pxd = cam->f * p->R[k] / oz - cam->f * ox / oz / oz * p->R[6 + k];
        double pyd = cam->f * p->R[3 + k] / oz - cam->f * oy / oz / oz * p->R[6 + k];
        out[k] = 0.5 / err * (2.0 * ex * -pxd + 2.0 * ey * -pyd);
    }
}

/* cv::Mat::inv(DECOMP_SVD) of a symmetric positive semi-definite 6x6 as an eigen-decomposition pseudo-inverse:
 * cyclic Jacobi (fixed 12 sweeps), eigenvalues <= 2*DBL_EPSILON*sum|w| are dropped */
XL_MATH_CALL_FN void pinv6(const double *A_, double *Ainv)
{
    double A[6][6], V[6][6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) { A[i][j] = A_[6 * i + j]; V[i][j] = (i == j) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 12; ++sweep)
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                double apq = A[p][q];
                if (apq == 0.0) continue;
                double tau = (A[q][q] - A[p][p]) / (2.0 * apq);
                double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < 6; ++k) {
                    double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 6; ++k) {
                    double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 6; ++k) {
                    double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    double sum = 0.0;
    for (int i = 0; i < 6; ++i) sum += fabs(A[i][i]);
    double thr = sum * (2.0 * XLM_DBL_EPS);
    double wi[6];
    for (int i = 0; i < 6; ++i) wi[i] = (fabs(A[i][i]) > thr) ? 1.0 / A[i][i] : 0.0;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
            for (int k = 0; k < 6; ++k) v += V[i][k] * wi[k] * V[j][k];
            Ainv[6 * i + j] = v;
        }
}

/* ground truth from a float 4x4 cam->world pose.  trans2pose (dsacstar_util.h:777-790) as a rigid inverse: the
 * reference passes the rotation through cv::Rodrigues and back (dsacstar_loss.h:107-108), which makes it exactly
 * orthonormal; float ground truth is not, and trace(R1 R2^T) > 3 would otherwise hit the clamp where the angle
 * derivative is infinite. */
XL_MATH_CALL_FN void gt_from_pose16(const float *gt16, Gt *g)
{
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) g->Rc2w[3 * i + j] = (double)gt16[4 * i + j];
        g->C[i] = (double)gt16[4 * i + 3];
    }
    double Rt[9], r2[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rt[3 * i + j] = g->Rc2w[3 * j + i];
    log_so3(Rt, r2);
    exp_so3(r2, g->R2);
    for (int i = 0; i < 3; ++i)
        g->t2[i] = -(g->R2[3 * i] * g->C[0] + g->R2[3 * i + 1] * g->C[1] + g->R2[3 * i + 2] * g->C[2]);
}

/* loss(pose2trans(est), gtTrans), dsacstar_loss.h:47-88.  estTrans = [R t]^-1: rot1 = R^T, centre c1 = -R^T t;
 * rotDiff = rot2 * rot1^T = Rc2w * R */
XL_MATH_CALL_FN double pose_loss(const Pose *est, const Gt *g, double wRot, double wTrans, double cut)
{
    double trace = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) trace += g->Rc2w[3 * i + k] * est->R[3 * k + i];
    trace = trace > 3.0 ? 3.0 : (trace < -1.0 ? -1.0 : trace);
    double rotErr = 180.0 * det_acos((trace - 1.0) / 2.0) / XLM_PI_REF;
    double d2 = 0.0;
    for (int i = 0; i < 3; ++i) {
        double c1 = -(est->R[i] * est->t[0] + est->R[3 + i] * est->t[1] + est->R[6 + i] * est->t[2]);
        double d = c1 - g->C[i];
        d2 += d * d;
    }
    double tErr = sqrt(d2);
    double loss = wRot * rotErr + wTrans * tErr;
    if (loss > cut) loss = sqrt(cut * loss);
    return loss < XLM_MAX_LOSS ? loss : XLM_MAX_LOSS;
}

/* dLoss, dsacstar_loss.h:99-212: 1x6 derivative w.r.t. (rvec, tvec) of the estimate; dR = rodrigues jacobian at it */
XL_MATH_CALL_FN void dloss(const Pose *est, const double *dR, const Gt *g, double wRot, double wTrans, double cut,
                           double *jac)
{
    for (int i = 0; i < 6; ++i) jac[i] = 0.0;
    const double *R1 = est->R, *R2 = g->R2;
    double trace = 0.0;                                  /* trace(R1 * R2^T) */
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k < 3; ++k) trace += R1[3 * a + k] * R2[3 * a + k];
    trace = trace > 3.0 ? 3.0 : (trace < -1.0 ? -1.0 : trace);
    double rotErr = 180.0 * det_acos((trace - 1.0) / 2.0) / XLM_CV_PI;
    double invT1[3], invT2[3], diff[3];
    for (int i = 0; i < 3; ++i) {
        invT1[i] = R1[i] * est->t[0] + R1[3 + i] * est->t[1] + R1[6 + i] * est->t[2];
        invT2[i] = R2[i] * g->t2[0] + R2[3 + i] * g->t2[1] + R2[6 + i] * g->t2[2];
        diff[i] = invT1[i] - invT2[i];
    }
    double tErr = sqrt(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]);
    double loss = wRot * rotErr + wTrans * tErr;
    int cutLoss = 0;
    if (loss > cut) { loss = sqrt(loss); cutLoss = 1; }
    if (loss > XLM_MAX_LOSS) return;
    if ((tErr + rotErr) < XLM_EPS) return;
    double dD[3];
    for (int i = 0; i < 3; ++i) dD[i] = diff[i] / tErr;
    /* translation part: dDist_dInvT1 * invRot1 */
    for (int j = 0; j < 3; ++j)
        jac[3 + j] += (dD[0] * R1[j * 3 + 0] + dD[1] * R1[j * 3 + 1] + dD[2] * R1[j * 3 + 2]) * wTrans;
    /* rotation through invT1 = R1^T t1: d invT1_i / d R1[j][i] = t1_j */
    for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) v += dD[i] * est->t[j] * dR[(3 * j + i) * 3 + c];
        jac[c] += v * wTrans;
    }
    /* rotation angle: d trace / d R1[a][k] = R2[a][k] */
    double fac = 180.0 / XLM_CV_PI * -1.0 / sqrt(3.0 - trace * trace + 2.0 * trace);
    for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int m = 0; m < 9; ++m) v += R2[m] * dR[m * 3 + c];
        jac[c] += fac * v * wRot;
    }
    if (cutLoss)
        for (int i = 0; i < 6; ++i) jac[i] *= 0.5 / loss;
    /* the reference tests for NaN only (loss.h:207-208); an infinite entry (estimate == ground truth to rounding,
     * where d acos is unbounded) would turn into NaN one product later, so it is treated the same way here */
    for (int i = 0; i < 6; ++i)
        if (!(jac[i] == jac[i]) || fabs(jac[i]) > 1.0e300) { for (int k = 0; k < 6; ++k) jac[k] = 0.0; return; }
}

#endif  /* XL_DSAC_MATH_H */
