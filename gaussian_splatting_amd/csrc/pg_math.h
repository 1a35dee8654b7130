// pg_math.h -- per-Gaussian device math shared by the stand-alone kernels (per_gaussian.hip) and the
// fused preprocess kernels (preprocess.hip).  Forward functions keep the reference's operation order
// (bit-identical fp32 results); see gs_common.h for the arithmetic contract.
#pragma once
#include "gs_common.h"

namespace gs {

template <typename T>
__device__ inline void quat_to_rot(T qw, T qx, T qy, T qz, T* R) {   // projection.cu:72-80
    R[0] = 1 - 2 * qy * qy - 2 * qz * qz;
    R[1] = 2 * qx * qy - 2 * qz * qw;
    R[2] = 2 * qx * qz + 2 * qy * qw;
    R[3] = 2 * qx * qy + 2 * qz * qw;
    R[4] = 1 - 2 * qx * qx - 2 * qz * qz;
    R[5] = 2 * qy * qz - 2 * qx * qw;
    R[6] = 2 * qx * qz - 2 * qy * qw;
    R[7] = 2 * qy * qz + 2 * qx * qw;
    R[8] = 1 - 2 * qx * qx - 2 * qy * qy;
}

// projection.cu:57-109
template <typename T>
__device__ inline void sigma_world_of(const T* q4, const T* s3, T* S) {
    T qw = q4[0], qx = q4[1], qy = q4[2], qz = q4[3];
    const T norm = gsqrt<T>(qx * qx + qy * qy + qz * qz + qw * qw);
    qx /= norm; qy /= norm; qz /= norm; qw /= norm;
    T r[9];
    quat_to_rot(qw, qx, qy, qz, r);
    const T sx = gexp<T>(s3[0]), sy = gexp<T>(s3[1]), sz = gexp<T>(s3[2]);
    const T sx2 = sx * sx, sy2 = sy * sy, sz2 = sz * sz;
    S[0] = r[0] * r[0] * sx2 + r[1] * r[1] * sy2 + r[2] * r[2] * sz2;
    S[1] = r[0] * r[3] * sx2 + r[1] * r[4] * sy2 + r[2] * r[5] * sz2;
    S[2] = r[0] * r[6] * sx2 + r[1] * r[7] * sy2 + r[2] * r[8] * sz2;
    S[3] = S[1];
    S[4] = r[3] * r[3] * sx2 + r[4] * r[4] * sy2 + r[5] * r[5] * sz2;
    S[5] = r[3] * r[6] * sx2 + r[4] * r[7] * sy2 + r[5] * r[8] * sz2;
    S[6] = S[2];
    S[7] = S[5];
    S[8] = r[6] * r[6] * sx2 + r[7] * r[7] * sy2 + r[8] * r[8] * sz2;
}


template <typename T>
__device__ inline void load_rotation(const T* __restrict__ M, T* W) {   // projection.cu:226-235
    W[0] = M[0]; W[1] = M[1]; W[2] = M[2];
    W[3] = M[4]; W[4] = M[5]; W[5] = M[6];
    W[6] = M[8]; W[7] = M[9]; W[8] = M[10];
}

// utils.py:60-72 as explicit fp32 arithmetic: ((m0*x + m1*y) + m2*z) + m3
__device__ inline void to_camera(const float* __restrict__ M, float x, float y, float z, float* c) {
    c[0] = M[0] * x + M[1] * y + M[2] * z + M[3];
    c[1] = M[4] * x + M[5] * y + M[6] * z + M[7];
    c[2] = M[8] * x + M[9] * y + M[10] * z + M[11];
}

// projection.cu:214-257
template <typename T>
__device__ inline void conic_of(const T* J6, const T* W, const T* S9, T* conic3) {
    T JW[6], JWS[6], JWt[6], S2[4];
    matmul<T, 2, 3, 3>(J6, W, JW);
    matmul<T, 2, 3, 3>(JW, S9, JWS);
    transp<T, 2, 3>(JW, JWt);
    matmul<T, 2, 3, 2>(JWS, JWt, S2);
    conic3[0] = S2[0];
    conic3[1] = S2[1] + S2[2];
    conic3[2] = S2[3];
}


// The gradient of (J W)^T [3,2] in the conic's backward: S (JW)^T G + S^T (JW)^T G
// (projection_backward.cu:430-455).  One definition for conic_bwd_of and conic_bwd_pose_of.
template <typename T>
__device__ inline void conic_bwd_gJWt_of(const T* JWt, const T* G2, const T* S9, T* gJWt) {
    T SJ[6], L[6], St[9], StJ[6], Rr[6];
    matmul<T, 3, 3, 2>(S9, JWt, SJ);
    matmul<T, 3, 2, 2>(SJ, G2, L);   // G2 is symmetric: its transpose is itself
    transp<T, 3, 3>(S9, St);
    matmul<T, 3, 3, 2>(St, JWt, StJ);
    matmul<T, 3, 2, 2>(StJ, G2, Rr);
#pragma unroll
    for (int k = 0; k < 6; k++) gJWt[k] = L[k] + Rr[k];
}

// projection_backward.cu:385-471
template <typename T>
__device__ inline void conic_bwd_of(const T* J6, const T* W, const T* S9, const T* gc3, T* gS9,
                                    T* gJ6) {
    T JW[6], JWt[6], G2[4], A[6], gJWt[6], gJt[6];
    matmul<T, 2, 3, 3>(J6, W, JW);
    transp<T, 2, 3>(JW, JWt);
    G2[0] = gc3[0]; G2[1] = gc3[1]; G2[2] = gc3[1]; G2[3] = gc3[2];
    matmul<T, 3, 2, 2>(JWt, G2, A);
    matmul<T, 3, 2, 3>(A, JW, gS9);
    conic_bwd_gJWt_of(JWt, G2, S9, gJWt);
    matmul<T, 3, 3, 2>(W, gJWt, gJt);
    transp<T, 3, 2>(gJt, gJ6);
}

// The conic's backward towards the camera pose: gJ6 as conic_bwd_of gives it, and gW9 [3,3], the gradient of the
// rotation block W through the product J W itself: J^T (gJWt)^T = 2 J^T G (J W) S for a symmetric S.  (The
// reference's ComputeConic returns no gradient for camera_T_world; this is the term it leaves out.)
template <typename T>
__device__ inline void conic_bwd_pose_of(const T* J6, const T* W, const T* S9, const T* gc3, T* gJ6,
                                         T* gW9) {
    T JW[6], JWt[6], G2[4], gJWt[6], gJt[6], Jt[6], gJW[6];
    matmul<T, 2, 3, 3>(J6, W, JW);
    transp<T, 2, 3>(JW, JWt);
    G2[0] = gc3[0]; G2[1] = gc3[1]; G2[2] = gc3[1]; G2[3] = gc3[2];
    conic_bwd_gJWt_of(JWt, G2, S9, gJWt);
    matmul<T, 3, 3, 2>(W, gJWt, gJt);
    transp<T, 3, 2>(gJt, gJ6);
    transp<T, 2, 3>(J6, Jt);
    transp<T, 3, 2>(gJWt, gJW);
    matmul<T, 3, 2, 3>(Jt, gJW, gW9);
}

// J and uv -> camera-frame xyz (projection_backward.cu:93-120 and :9-36; the uv part is nothing when z <= 0, Q10).
// c: the camera-frame position, gJ6: the gradient of the projection Jacobian, g_uv: the gradient of uv (read only
// when z > 0).
template <typename T>
__device__ inline void cam_grad_of(const T* c, T fx, T fy, const T* gJ6, const T* g_uv, T* gcam) {
    const T z = c[2], z2 = c[2] * c[2], z3 = c[2] * c[2] * c[2];
    gcam[0] = gJ6[2] * -fx / z2;
    gcam[1] = gJ6[5] * -fy / z2;
    gcam[2] = gJ6[0] * -fx / z2 + gJ6[4] * -fy / z2 + gJ6[2] * 2 * c[0] * fx / z3 +
              gJ6[5] * 2 * c[1] * fy / z3;
    if (z > T(0)) {
        const T gu = g_uv[0], gv = g_uv[1];
        gcam[0] += gu * (fx / z);
        gcam[1] += gv * (fy / z);
        gcam[2] += gu * (-fx * c[0] / z2) + gv * (-fy * c[1] / z2);
    }
}


// ---- equidistant fisheye camera (GS_RASTER_FISHEYE; include/gsplat_hip.h "fisheye camera") ----
// With c = (x, y, z) the camera-frame position (to_camera, as for the pinhole model):
//     r2 = x x + y y      q = 1 / (r2 + z z)      r = sqrt(r2)      theta = atan2(r, z)
//     s = theta / r                       (r2 == 0, the optical axis: s = 1 / z)
//     a = (z q - s) / r2                  (d s / d x = a x,  d s / d y = a y,  d s / d z = -q)
//     d = -(2 z q q + 3 a) / r2           (d a / d x = d x,  d a / d y = d y,  d a / d z = 2 q q)
//     u = fx s x + cx     v = fy s y + cy
//     J = [[fx (s + x x a),  fx x y a,        -fx x q],
//          [fy x y a,        fy (s + y y a),  -fy y q]]
// fp32, no contraction, IEEE divide and square root; atan2f is the device library's (no reference restatement exists
// for this model; the fp64 yardstick of tests/fisheye_ref.py bounds it).
// a and d cancel near the axis: z q -> s leaves a with an absolute error ~ 2^-24 / (z r2), harmless in J (a is
// multiplied by x x, x y, y y) but not in the backward, whose terms 3 a x and x^3 d then carry a relative error
// ~ 2^-24 z^2 / r2.  So for w = r2 / z^2 < 1/16 (theta < 14 degrees, the exact axis included) a and d are their series
//     a z^3 = sum_{k>=1} (-1)^k 2k / (2k + 1) w^(k-1) = -2/3 + 4/5 w - 6/7 w^2 + ...          (eight terms)
//     d z^5 / 2 = sum_{k>=2} (-1)^k 2k (k - 1) / (2k + 1) w^(k-2) = 4/5 - 12/7 w + 24/9 w^2 - ...   (seven terms)
// in Horner form (truncation < 2^-24 of the sum), the limits a = -2 / (3 z^3), d = 8 / (5 z^5) at w = 0; beyond, the
// closed forms are within ~1e-6 relative (the optical-axis rows of tests/test_gpu_fisheye.py).
// The forward (is_culled, k_preprocess) and both backwards (k_preprocess_bwd, k_pose_bwd) call these functions.
struct FisheyeTerms {
    float s, a, q, d;
};
__device__ inline FisheyeTerms fisheye_terms_of(const float* c) {
    FisheyeTerms t;
    const float x = c[0], y = c[1], z = c[2];
    const float r2 = x * x + y * y, z2 = z * z;
    t.q = 1.0f / (r2 + z2);
    if (r2 > 0.0f) {
        const float r = __builtin_sqrtf(r2);
        t.s = ::atan2f(r, z) / r;
    } else {
        t.s = 1.0f / z;
    }
    if (r2 < 0.0625f * z2) {
        const float w = r2 / z2, z3 = z2 * z;
        float fa = 16.0f / 17.0f, fd = 112.0f / 17.0f;
        fa = fa * w + -14.0f / 15.0f;   fd = fd * w + -84.0f / 15.0f;
        fa = fa * w + 12.0f / 13.0f;    fd = fd * w + 60.0f / 13.0f;
        fa = fa * w + -10.0f / 11.0f;   fd = fd * w + -40.0f / 11.0f;
        fa = fa * w + 8.0f / 9.0f;      fd = fd * w + 24.0f / 9.0f;
        fa = fa * w + -6.0f / 7.0f;     fd = fd * w + -12.0f / 7.0f;
        fa = fa * w + 4.0f / 5.0f;      fd = fd * w + 4.0f / 5.0f;
        fa = fa * w + -2.0f / 3.0f;
        t.a = fa / z3;
        t.d = 2.0f * fd / (z3 * z2);
    } else {
        t.a = (z * t.q - t.s) / r2;
        t.d = -(2.0f * z * t.q * t.q + 3.0f * t.a) / r2;
    }
    return t;
}

__device__ inline void fisheye_project(const float* c, const FisheyeTerms& t, float fx, float fy, float cx, float cy,
                                       float* uv) {
    uv[0] = fx * t.s * c[0] + cx;
    uv[1] = fy * t.s * c[1] + cy;
}

__device__ inline void fisheye_J6_of(const float* c, const FisheyeTerms& t, float fx, float fy, float* J6) {
    const float x = c[0], y = c[1];
    const float xya = x * y * t.a;
    J6[0] = fx * (t.s + x * x * t.a);
    J6[1] = fx * xya;
    J6[2] = -fx * x * t.q;
    J6[3] = fy * xya;
    J6[4] = fy * (t.s + y * y * t.a);
    J6[5] = -fy * y * t.q;
}

// The fisheye twin of cam_grad_of: J (all six entries) and uv -> camera-frame xyz.  The uv part is g_uv^T J, read only
// when z > 0 as there.  d J / d c from the derivatives listed above:
//     dJ0 = fx (3 a x + x^3 d,   a y + x x y d,   2 x x q q - q)      dJ1 = fx (a y + x x y d,  a x + x y y d,  2 x y q q)
//     dJ4 = fy (a x + x y y d,   3 a y + y^3 d,   2 y y q q - q)      dJ3 = dJ1 fy / fx
//     dJ2 = fx (2 x x q q - q,   2 x y q q,       2 x z q q)          dJ5 = fy (2 x y q q,  2 y y q q - q,  2 y z q q)
__device__ inline void fisheye_cam_grad_of(const float* c, const FisheyeTerms& t, float fx, float fy, const float* gJ6,
                                           const float* g_uv, float* gcam) {
    const float x = c[0], y = c[1], z = c[2];
    const float a = t.a, d = t.d, q = t.q, qq2 = 2.0f * t.q * t.q;
    const float ax = a * x, ay = a * y;
    const float xxyd = x * x * y * d, xyyd = x * y * y * d;
    const float zxx = x * x * qq2 - q, zyy = y * y * qq2 - q, zxy = x * y * qq2;
    const float g0 = gJ6[0] * fx, g1 = gJ6[1] * fx + gJ6[3] * fy, g2 = gJ6[2] * fx;
    const float g4 = gJ6[4] * fy, g5 = gJ6[5] * fy;
    gcam[0] = g0 * (3.0f * ax + x * x * x * d) + g1 * (ay + xxyd) + g4 * (ax + xyyd) + g2 * zxx + g5 * zxy;
    gcam[1] = g0 * (ay + xxyd) + g1 * (ax + xyyd) + g4 * (3.0f * ay + y * y * y * d) + g2 * zxy + g5 * zyy;
    gcam[2] = g0 * zxx + g1 * zxy + g4 * zyy + g2 * (x * z * qq2) + g5 * (y * z * qq2);
    if (z > 0.0f) {
        float J6[6];
        fisheye_J6_of(c, t, fx, fy, J6);
        const float gu = g_uv[0], gv = g_uv[1];
        gcam[0] += gu * J6[0] + gv * J6[3];
        gcam[1] += gu * J6[1] + gv * J6[4];
        gcam[2] += gu * J6[2] + gv * J6[5];
    }
}

// precompute_sh.cu:28-39 ; rsqrt -> 1/sqrt (IEEE)
template <typename T>
__device__ inline void view_dir_of(const T* __restrict__ xyz, const T* __restrict__ M, int g,
                                   T* d) {
    d[0] = xyz[g * 3 + 0] - M[3];
    d[1] = xyz[g * 3 + 1] - M[7];
    d[2] = xyz[g * 3 + 2] - M[11];
    const T r = T(1) / gsqrt<T>(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    d[0] *= r; d[1] *= r; d[2] *= r;
}


// Conservative squared cutoff radius of a splat for the fp32 alpha threshold (render.cu:145):
// alpha >= 1/255  <=>  mh^2 <= tau = 2 ln(255 opacity), and mh^2 = d' S^-1 d >= |d|^2 / lmax(S),
// so |d|^2 > tau * lmax  =>  alpha < 1/255.  The margin covers the rounding of the fp32
// quadratic form (relative error ~ condition number * 2^-24) and of log/exp; parity tests against
// the oracle (which evaluates every pixel) are bit-exact, so any non-conservative case would show.
__device__ inline float cutoff_r2(float a, float b, float c, float det, float opa) {
    if (!(det > 0.0f) || !(a > 0.0f) || !(c > 0.0f) || !(opa == opa)) return __builtin_inff();
    const float s = opa * 255.0f * 1.001f;   // margin: opacity within rounding of 1/255
    if (!(s > 1.0f)) return -1.0f;           // alpha <= opacity < 1/255 everywhere
    const float tau = 2.0f * __builtin_logf(s);
    const float half = 0.5f * (a + c);
    const float lmax = half + __builtin_sqrtf(0.25f * (a - c) * (a - c) + b * b);
    const float kappa = lmax * lmax / det;   // lmax / lmin
    return tau * lmax * (1.05f + 8e-6f * kappa) + 1e-3f;
}
template <typename T> __device__ inline T cutoff_r2_t(T a, T b, T c, T det, T opa);
template <> __device__ inline float cutoff_r2_t<float>(float a, float b, float c, float det, float opa) {
    return cutoff_r2(a, b, c, det, opa);
}
template <> __device__ inline double cutoff_r2_t<double>(double, double, double, double, double) {
    return (double)__builtin_inff();   // fp64 has no alpha threshold (render.cu:145: use_fast_exp)
}

// the packed render record (gs_pack_splats): the per-splat part of the per-pixel loop of
// render.cu:117-129 / render_backward.cu:141-152, hoisted (identical values)
template <typename T>
__device__ inline void pack_record(T u, T v, const T* conic3, T opa, const T* col3, T* p) {
    constexpr bool fast = sizeof(T) == 4;
    T a, c;
    const T b = conic3[1] * 0.5;
    if (fast) {
        a = conic3[0] + 0.25;
        c = conic3[2] + 0.25;
    } else {
        a = conic3[0];
        c = conic3[2];
    }
    const T det = a * c - b * b;
    const T rdet = 1.0 / det;
    p[0] = u; p[1] = v; p[2] = cutoff_r2_t<T>(a, b, c, det, opa); p[3] = opa;
    p[4] = a; p[5] = b; p[6] = c; p[7] = det;
    p[8] = rdet;
    // the splat's colour as the render loops use it with one coefficient per channel: sh_to_rgb's
    // Y0 * coefficient (spherical_harmonics.cuh:83), the same product formed once per splat
    p[9] = col3 ? T(GS_SH_0) * col3[0] : T(0);
    p[10] = col3 ? T(GS_SH_0) * col3[1] : T(0);
    p[11] = col3 ? T(GS_SH_0) * col3[2] : T(0);
}

// ---- antialiased opacity (GS_RASTER_ANTIALIASED; include/gsplat_hip.h "antialiased opacity") ----
// The fp32 record dilates Sigma_2D by 0.25 px^2 and leaves the opacity alone; the factor comp = sqrt(det Sigma_2D /
// det(Sigma_2D + 0.25 I)) keeps a splat's integrated weight independent of the dilation.  a, b, c, det_d are the
// expressions of pack_record on the same bits (det_d == packed[7]); IEEE divide and square root; a NaN compares false
// and gives comp = 0.  The forward (k_preprocess) and both backwards (k_preprocess_bwd, k_pose_bwd) call this one
// function on the conic conic_of gives them.
struct AaTerms {
    float a0, c0, b, a, c, det_0, det_d, comp;
};
__device__ inline AaTerms aa_terms_of(const float* conic3) {
    AaTerms t;
    t.a0 = conic3[0];
    t.c0 = conic3[2];
    t.b = conic3[1] * 0.5;
    t.a = conic3[0] + 0.25;
    t.c = conic3[2] + 0.25;
    t.det_d = t.a * t.c - t.b * t.b;
    t.det_0 = t.a0 * t.c0 - t.b * t.b;
    const float rho = t.det_0 / t.det_d;
    t.comp = (t.det_0 > 0.0f && t.det_d > 0.0f) ? __builtin_sqrtf(rho) : 0.0f;
    return t;
}

// The backward of opa_eff = y * comp folded into one row of the render-gradient slab, in registers: g = dL/d opa_eff
// (slab column 3) becomes dL/dy, and the conic columns gain dL/d opa_eff * y * d comp / d conic -- the true derivative,
// no epsilon (d comp / d rho = 0.5 / comp grows without bound as det_0 cancels; comp == 0 rows get nothing).
// WIDE (the F3D instantiations): a filter can make a splat millions of pixels wide, and from det_d ~ 1e19 on det_d^2 and
// c0 det_d leave fp32's range (inf / inf).  Beyond det_d > 1e18 the same three terms are formed as (c0 - rho c) / det_d,
// b (rho - 1) / det_d, (a0 - rho a) / det_d, whose products stay finite; below, the expressions -- and bits -- are the
// ones every other instantiation has.  (A wider band, not every magnitude: from conic ~ 1e19 det_0 and det_d are infinite
// themselves and comp = sqrt(inf / inf) is not a number, as in 7e without a filter.  tests/test_gpu_filter3d.py puts rows on both sides of the threshold.)
template <bool WIDE = false>
__device__ inline void aa_fold_row(const AaTerms& t, float y, float& g_opa, float* gc3) {
    const float g = g_opa;
    g_opa = g * t.comp;
    if (t.comp > 0.0f) {
        const float g_rho = g * y * 0.5f / t.comp;
        if constexpr (WIDE) {
            if (t.det_d > 1e18f) {
                const float rho = t.det_0 / t.det_d;
                gc3[0] += g_rho * (t.c0 - rho * t.c) / t.det_d;
                gc3[1] += g_rho * t.b * (rho - 1.0f) / t.det_d;
                gc3[2] += g_rho * (t.a0 - rho * t.a) / t.det_d;
                return;
            }
        }
        const float dd = t.det_d * t.det_d;
        gc3[0] += g_rho * (t.c0 * t.det_d - t.det_0 * t.c) / dd;
        gc3[1] += g_rho * t.b * (t.det_0 - t.det_d) / dd;   // conic1 = 2 b
        gc3[2] += g_rho * (t.a0 * t.det_d - t.det_0 * t.a) / dd;
    }
}

// ---- 3D smoothing filter (the filter3d argument of the _filtered entries; include/gsplat_hip.h "3D smoothing filter",
// DESIGN.md 7k) ----
// phi >= 0 is a per-Gaussian world-space variance, a constant of the frame.  The filter is isotropic:
// R diag(s^2 + phi) R^T = Sigma + phi I, so the forward adds phi to the diagonal of what sigma_world_of returned and the
// covariance's gradient passes through sigma_world_bwd_of on the unfiltered scale unchanged.  With s_k = exp(scale_k)
// (sigma_world_of's expression, squared as there):
//     rho3  = ((s_0^2 / (s_0^2 + phi)) * (s_1^2 / (s_1^2 + phi))) * (s_2^2 / (s_2^2 + phi))
//     comp3 = rho3 > 0 ? sqrt(rho3) : 0                     (a NaN compares false)
//     opa3  = sigmoid(opacity) * comp3                      (what the record, and comp of 7e, multiply)
//     d opa3 / d scale_k = opa3 phi / (s_k^2 + phi)         (no epsilon; a comp3 == 0 row gets no term)
// fp32, no contraction, IEEE divide and square root.  With phi == 0 every step is exact (x + 0, s^2 / s^2 = 1, sqrt(1) = 1,
// y * 1, + 0): such a row carries the values of the call without a filter.  The forward (k_preprocess) and both backwards
// (k_preprocess_bwd, k_pose_bwd) call these functions.
__device__ inline void filter3d_sigma(float* S9, float phi) {
    S9[0] += phi;
    S9[4] += phi;
    S9[8] += phi;
}

// comp3 and the three denominators d[k] = s_k^2 + phi, the exponentials evaluated once
struct F3dTerms {
    float comp3, d[3];
};
__device__ inline F3dTerms filter3d_terms_of(const float* s3, float phi) {
    F3dTerms t;
    float rho3 = 1.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float e = gexp<float>(s3[k]);
        const float s2 = e * e;
        t.d[k] = s2 + phi;
        rho3 *= s2 / t.d[k];
    }
    t.comp3 = rho3 > 0.0f ? __builtin_sqrtf(rho3) : 0.0f;
    return t;
}
__device__ inline float filter3d_comp_of(const float* s3, float phi) { return filter3d_terms_of(s3, phi).comp3; }

// The backward of opa3 = y comp3 for g_opa3 = dL/d opa3: -> the opacity-logit gradient, and ts[k] = the term the scale
// gradient gains, g_opa3 opa3 phi / (s_k^2 + phi); zeros for a comp3 == 0 row.  Formed where the caller has the terms, ahead
// of the covariance's backward: three values cross it instead of phi, comp3, y and g_opa3.
__device__ inline float filter3d_bwd_of(const F3dTerms& t, float phi, float y, float g_opa3, float* ts) {
    ts[0] = ts[1] = ts[2] = 0.0f;
    if (!(t.comp3 > 0.0f)) return 0.0f;
    const float num = g_opa3 * (y * t.comp3) * phi;
#pragma unroll
    for (int k = 0; k < 3; k++) ts[k] = num / t.d[k];
    return g_opa3 * t.comp3 * (1.0f - y) * y;
}

// projection_backward.cu:174-315
template <typename T>
__device__ inline void sigma_world_bwd_of(const T* q4, const T* s3, const T* G, T* g_q4, T* g_s3) {
    const T e0 = gexp<T>(s3[0]), e1 = gexp<T>(s3[1]),
            e2 = gexp<T>(s3[2]);
    const T S[9] = {e0, 0, 0, 0, e1, 0, 0, 0, e2};
    const T qw = q4[0], qx = q4[1], qy = q4[2], qz = q4[3];
    const T norm_q = gsqrt<T>(qw * qw + qx * qx + qy * qy + qz * qz);
    const T w = qw / norm_q, x = qx / norm_q, y = qy / norm_q, z = qz / norm_q;
    T R[9];
    quat_to_rot(w, x, y, z, R);
    T RS[9], gradRS[9], RSt[9], gradSR[9], gradR[9], SgradSR[9], Rt[9], gradS[9], gradSRR[9];
    matmul<T, 3, 3, 3>(R, S, RS);
    matmul<T, 3, 3, 3>(G, RS, gradRS);
    transp<T, 3, 3>(RS, RSt);
    matmul<T, 3, 3, 3>(RSt, G, gradSR);
    matmul<T, 3, 3, 3>(gradRS, S, gradR);
    matmul<T, 3, 3, 3>(S, gradSR, SgradSR);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) gradR[r * 3 + c] += SgradSR[c * 3 + r];
    transp<T, 3, 3>(R, Rt);
    matmul<T, 3, 3, 3>(Rt, gradRS, gradS);
    matmul<T, 3, 3, 3>(gradSR, R, gradSRR);
    g_s3[0] = (gradS[0] + gradSRR[0]) * e0;
    g_s3[1] = (gradS[4] + gradSRR[4]) * e1;
    g_s3[2] = (gradS[8] + gradSRR[8]) * e2;
    T gq[4];
    gq[0] = -2 * z * gradR[1] + 2 * y * gradR[2] + 2 * z * gradR[3] - 2 * x * gradR[5] -
            2 * y * gradR[6] + 2 * x * gradR[7];
    gq[1] = 2 * y * gradR[1] + 2 * z * gradR[2] + 2 * y * gradR[3] - 4 * x * gradR[4] -
            2 * w * gradR[5] + 2 * z * gradR[6] + 2 * w * gradR[7] - 4 * x * gradR[8];
    gq[2] = -4 * y * gradR[0] + 2 * x * gradR[1] + 2 * w * gradR[2] + 2 * x * gradR[3] +
            2 * z * gradR[5] - 2 * w * gradR[6] + 2 * z * gradR[7] - 4 * y * gradR[8];
    gq[3] = -4 * z * gradR[0] - 2 * w * gradR[1] + 2 * x * gradR[2] + 2 * w * gradR[3] -
            4 * z * gradR[4] + 2 * y * gradR[5] + 2 * x * gradR[6] + 2 * y * gradR[7];
    const T n3 = norm_q * norm_q * norm_q;
    const T inv = T(1) / norm_q;
    g_q4[0] = (inv - qw * qw / n3) * gq[0] - qw * qx / n3 * gq[1] - qw * qy / n3 * gq[2] -
                     qw * qz / n3 * gq[3];
    g_q4[1] = -qw * qx / n3 * gq[0] + (inv - qx * qx / n3) * gq[1] - qx * qy / n3 * gq[2] -
                     qx * qz / n3 * gq[3];
    g_q4[2] = -qw * qy / n3 * gq[0] - qx * qy / n3 * gq[1] + (inv - qy * qy / n3) * gq[2] -
                     qy * qz / n3 * gq[3];
    g_q4[3] = -qw * qz / n3 * gq[0] - qx * qz / n3 * gq[1] - qy * qz / n3 * gq[2] +
                     (inv - qz * qz / n3) * gq[3];
}

}  // namespace gs
