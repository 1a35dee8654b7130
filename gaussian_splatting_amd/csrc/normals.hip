// normals.hip -- what the normal-consistency regulariser needs around the feature walk (include/gsplat_hip.h "Normals",
// DESIGN.md 7l): the visible Gaussians' normals in the camera frame, and the normal of a rendered depth map.
//
//   k_gaussian_normals       one thread per visible row: the normalised quaternion's rotation, the column of the
//                            smallest log-scale, the camera's rotation, the flip towards the camera.  56 B per row.
//   k_gaussian_normals_bwd   one thread per Gaussian of the N, through rank: grad_normals -> grad_quaternion with the
//                            axis and the flip as constants; culled rows are written as zeros.  No atomics.
//   k_depth_normal           one 16x16 tile per workgroup: the back-projected points of the tile and a halo of 1 are
//                            staged in LDS (one ray evaluation per staged pixel, not five), then one cross product per pixel.
//   k_depth_normal_bwd       a gather: points with a halo of 2, then the two stencil-difference gradients of every centre
//                            of the tile and a halo of 1 (LDS again), then each pixel sums the four centres whose stencil
//                            holds it.  No atomics: two runs are bit-equal.
//
// An invalid back-projection (alpha <= min_alpha, a fisheye ray at or beyond 90 degrees, a pixel outside the image) is
// staged as a NaN depth, so that every difference it enters is NaN and the one test "squared norm > 0" refuses the
// centre; the forward and the backward run the same function on the same values and so take the same decisions.
#include "pg_math.h"

namespace gs {

constexpr int NB_BLOCK = 256;

// steps 1-6 of the header's definition; -> the axis, and whether the normal was negated
struct NormalChoice {
    int axis;
    bool flip;
};
__device__ inline NormalChoice gaussian_normal_of(const float* q4, const float* s3, const float* W, const float* p_cam,
                                                  float* qhat, float* n_c) {
    float qw = q4[0], qx = q4[1], qy = q4[2], qz = q4[3];
    const float norm = __builtin_sqrtf(qx * qx + qy * qy + qz * qz + qw * qw);   // (sigma_world_of's expression)
    qx /= norm; qy /= norm; qz /= norm; qw /= norm;
    qhat[0] = qw; qhat[1] = qx; qhat[2] = qy; qhat[3] = qz;
    float R[9];
    quat_to_rot(qw, qx, qy, qz, R);
    NormalChoice c;
    c.axis = 0;
    float least = s3[0];
    if (s3[1] < least) { c.axis = 1; least = s3[1]; }
    if (s3[2] < least) c.axis = 2;
    const float n0 = c.axis == 0 ? R[0] : (c.axis == 1 ? R[1] : R[2]);
    const float n1 = c.axis == 0 ? R[3] : (c.axis == 1 ? R[4] : R[5]);
    const float n2 = c.axis == 0 ? R[6] : (c.axis == 1 ? R[7] : R[8]);
    n_c[0] = W[0] * n0 + W[1] * n1 + W[2] * n2;
    n_c[1] = W[3] * n0 + W[4] * n1 + W[5] * n2;
    n_c[2] = W[6] * n0 + W[7] * n1 + W[8] * n2;
    c.flip = n_c[0] * p_cam[0] + n_c[1] * p_cam[1] + n_c[2] * p_cam[2] > 0.0f;
    if (c.flip) { n_c[0] = -n_c[0]; n_c[1] = -n_c[1]; n_c[2] = -n_c[2]; }
    return c;
}

__global__ __launch_bounds__(NB_BLOCK) void k_gaussian_normals(const float* __restrict__ quaternion,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ cam,
                                                               const int* __restrict__ vis_idx,
                                                               const float* __restrict__ xyz_cam, int V,
                                                               float* __restrict__ normals) {
    const int v = blockIdx.x * NB_BLOCK + threadIdx.x;
    if (v >= V) return;
    const size_t i = (size_t)vis_idx[v];
    const float4 q = *reinterpret_cast<const float4*>(quaternion + i * 4);
    const float q4[4] = {q.x, q.y, q.z, q.w};
    const float s3[3] = {scale[i * 3 + 0], scale[i * 3 + 1], scale[i * 3 + 2]};
    const float p[3] = {xyz_cam[(size_t)v * 3 + 0], xyz_cam[(size_t)v * 3 + 1], xyz_cam[(size_t)v * 3 + 2]};
    float W[9], qhat[4], n[3];
    load_rotation(cam, W);
    gaussian_normal_of(q4, s3, W, p, qhat, n);
    normals[(size_t)v * 3 + 0] = n[0];
    normals[(size_t)v * 3 + 1] = n[1];
    normals[(size_t)v * 3 + 2] = n[2];
}

__global__ __launch_bounds__(NB_BLOCK) void k_gaussian_normals_bwd(const float* __restrict__ quaternion,
                                                                   const float* __restrict__ scale,
                                                                   const float* __restrict__ cam,
                                                                   const int* __restrict__ rank,
                                                                   const float* __restrict__ xyz_cam,
                                                                   const float* __restrict__ grad_normals, int V, int N,
                                                                   float* __restrict__ grad_quaternion) {
    const int i = blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= N) return;
    float4 out = {0.0f, 0.0f, 0.0f, 0.0f};
    const int v = rank[i];
    if (v >= 0 && v < V) {
        const float4 q = *reinterpret_cast<const float4*>(quaternion + (size_t)i * 4);
        const float q4[4] = {q.x, q.y, q.z, q.w};
        const float s3[3] = {scale[(size_t)i * 3 + 0], scale[(size_t)i * 3 + 1], scale[(size_t)i * 3 + 2]};
        const float p[3] = {xyz_cam[(size_t)v * 3 + 0], xyz_cam[(size_t)v * 3 + 1], xyz_cam[(size_t)v * 3 + 2]};
        float W[9], qh[4], n[3];
        load_rotation(cam, W);
        const NormalChoice c = gaussian_normal_of(q4, s3, W, p, qh, n);
        float g[3] = {grad_normals[(size_t)v * 3 + 0], grad_normals[(size_t)v * 3 + 1], grad_normals[(size_t)v * 3 + 2]};
        if (c.flip) { g[0] = -g[0]; g[1] = -g[1]; g[2] = -g[2]; }
        // n_c = W n_w: dL/dn_w = W^T g, the gradient of column `axis` of R; the other columns have none
        const float gw[3] = {W[0] * g[0] + W[3] * g[1] + W[6] * g[2], W[1] * g[0] + W[4] * g[1] + W[7] * g[2],
                             W[2] * g[0] + W[5] * g[1] + W[8] * g[2]};
        float gR[9];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int k = 0; k < 3; k++) gR[r * 3 + k] = c.axis == k ? gw[r] : 0.0f;
        // quat_to_rot's derivative (sigma_world_bwd_of's expressions) towards the normalised quaternion
        const float w = qh[0], x = qh[1], y = qh[2], z = qh[3];
        float gq[4];
        gq[0] = -2 * z * gR[1] + 2 * y * gR[2] + 2 * z * gR[3] - 2 * x * gR[5] - 2 * y * gR[6] + 2 * x * gR[7];
        gq[1] = 2 * y * gR[1] + 2 * z * gR[2] + 2 * y * gR[3] - 4 * x * gR[4] - 2 * w * gR[5] + 2 * z * gR[6] +
                2 * w * gR[7] - 4 * x * gR[8];
        gq[2] = -4 * y * gR[0] + 2 * x * gR[1] + 2 * w * gR[2] + 2 * x * gR[3] + 2 * z * gR[5] - 2 * w * gR[6] +
                2 * z * gR[7] - 4 * y * gR[8];
        gq[3] = -4 * z * gR[0] - 2 * w * gR[1] + 2 * x * gR[2] + 2 * w * gR[3] - 4 * z * gR[4] + 2 * y * gR[5] +
                2 * x * gR[6] + 2 * y * gR[7];
        // qhat = q / |q|: dL/dq = (gq - qhat (qhat . gq)) / |q|
        const float norm = __builtin_sqrtf(q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3] + q4[0] * q4[0]);
        const float along = w * gq[0] + x * gq[1] + y * gq[2] + z * gq[3];
        out.x = (gq[0] - w * along) / norm;
        out.y = (gq[1] - x * along) / norm;
        out.z = (gq[2] - y * along) / norm;
        out.w = (gq[3] - z * along) / norm;
    }
    *reinterpret_cast<float4*>(grad_quaternion + (size_t)i * 4) = out;
}

// ---- depth normals ----------------------------------------------------------------------------------------------------
constexpr int DN_TILE = 16;
// pi / 2 = DN_PIO2_HI + DN_PIO2_LO; DN_PIO2_HI is the float above pi / 2, so every theta below it is below pi / 2
constexpr float DN_PIO2_HI = 0x1.921fb6p+0f, DN_PIO2_LO = -0x1.777a5cp-25f, DN_PIO4 = 0x1.921fb6p-1f;

// tan(theta) / theta for 0 <= theta < pi / 2 from +, *, / alone (no library call), so that the float32 restatement of the
// tests (tests/normals_ref.py) repeats it operation for operation, as it does the pinhole ray.  With the Taylor series
// of sin(x) / x (to x^10) and cos(x) (to x^12) in Horner form on x <= pi / 4, where the first terms left out are under
// 1e-11 and 4e-13:
//     theta <= pi / 4    x = theta,                                (sin(x) / x) / cos(x)       -- no division by theta: 1 at the axis
//     beyond             x = (DN_PIO2_HI - theta) + DN_PIO2_LO,    (cos(x) / (x (sin(x) / x))) / theta
// within 2.6e-7 relative (measured; tests/test_normals_ref.py holds it to 4.8e-7) of the true value over the whole range (the difference DN_PIO2_HI - theta is exact).
__device__ inline float tan_over_theta(float theta) {
    const bool low = theta <= DN_PIO4;
    const float x = low ? theta : (DN_PIO2_HI - theta) + DN_PIO2_LO;
    const float x2 = x * x;
    float ps = -0x1.ae6456p-26f;          // -1 / 11!
    ps = ps * x2 + 0x1.71de3ap-19f;       //  1 / 9!
    ps = ps * x2 + -0x1.a01a02p-13f;      // -1 / 7!
    ps = ps * x2 + 0x1.111112p-7f;        //  1 / 5!
    ps = ps * x2 + -0x1.555556p-3f;       // -1 / 3!
    ps = ps * x2 + 1.0f;
    float pc = 0x1.1eed8ep-29f;           //  1 / 12!
    pc = pc * x2 + -0x1.27e4fcp-22f;      // -1 / 10!
    pc = pc * x2 + 0x1.a01a02p-16f;       //  1 / 8!
    pc = pc * x2 + -0x1.6c16c2p-10f;      // -1 / 6!
    pc = pc * x2 + 0x1.555556p-5f;        //  1 / 4!
    pc = pc * x2 + -0.5f;
    pc = pc * x2 + 1.0f;
    return low ? ps / pc : (pc / (x * ps)) / theta;
}

struct Intrinsics {
    float fx, fy, cx, cy;
};

// the direction (rx, ry, 1) whose multiple by d is the back-projection of pixel (x, y) at camera-frame depth d;
// -> false for a fisheye ray at or beyond 90 degrees
template <bool FISH>
__device__ inline bool ray_of(const Intrinsics& k, int x, int y, float& rx, float& ry) {
    rx = ((float)x - k.cx) / k.fx;
    ry = ((float)y - k.cy) / k.fy;
    if constexpr (FISH) {
        const float theta = __builtin_sqrtf(rx * rx + ry * ry);
        if (!(theta < DN_PIO2_HI)) return false;
        const float s = tan_over_theta(theta);
        rx *= s;
        ry *= s;
    }
    return true;
}

// the tile's back-projected points with a halo of HALO pixels, as three planes of EDGE x EDGE floats; an invalid one
// (see the head of the file) has a NaN z
template <bool FISH, int HALO>
__device__ inline void stage_points(const float* __restrict__ depth, const float* __restrict__ alpha, const Intrinsics& k,
                                    int W, int H, float min_alpha, int x0, int y0, float* sP) {
    constexpr int EDGE = DN_TILE + 2 * HALO, CELLS = EDGE * EDGE;
    for (int c = threadIdx.x; c < CELLS; c += NB_BLOCK) {
        const int x = x0 - HALO + c % EDGE, y = y0 - HALO + c / EDGE;
        float px = 0.0f, py = 0.0f, pz = __builtin_nanf("");
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t p = (size_t)y * W + x;
            const float a = alpha[p];
            float rx, ry;
            if (a > min_alpha && ray_of<FISH>(k, x, y, rx, ry)) {
                pz = depth[p] / a;
                px = pz * rx;
                py = pz * ry;
            }
        }
        sP[c] = px;
        sP[CELLS + c] = py;
        sP[2 * CELLS + c] = pz;
    }
}

// the stencil of the centre at cell c of the staged planes: a = P(x, y + 1) - P(x, y - 1), b = P(x + 1, y) - P(x - 1, y),
// cr = a x b -> its squared norm (NaN when the centre or a neighbour is invalid)
template <int EDGE>
__device__ inline float stencil_of(const float* sP, int c, float* a, float* b, float* cr) {
    constexpr int CELLS = EDGE * EDGE;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        a[j] = sP[j * CELLS + c + EDGE] - sP[j * CELLS + c - EDGE];
        b[j] = sP[j * CELLS + c + 1] - sP[j * CELLS + c - 1];
    }
    cr[0] = a[1] * b[2] - a[2] * b[1];
    cr[1] = a[2] * b[0] - a[0] * b[2];
    cr[2] = a[0] * b[1] - a[1] * b[0];
    const float n2 = cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2];
    return sP[2 * CELLS + c] == sP[2 * CELLS + c] ? n2 : __builtin_nanf("");   // (the centre itself must be valid)
}

__device__ inline Intrinsics intrinsics_of(const float* __restrict__ K) {
    Intrinsics k;
    k.fx = K[0]; k.fy = K[4]; k.cx = K[2]; k.cy = K[5];
    return k;
}

template <bool FISH>
__global__ __launch_bounds__(NB_BLOCK) void k_depth_normal(const float* __restrict__ depth,
                                                           const float* __restrict__ alpha, const float* __restrict__ K,
                                                           int W, int H, float min_alpha, float* __restrict__ normal) {
    constexpr int EDGE = DN_TILE + 2;
    __shared__ float sP[3 * EDGE * EDGE];
    const int x0 = blockIdx.x * DN_TILE, y0 = blockIdx.y * DN_TILE;
    stage_points<FISH, 1>(depth, alpha, intrinsics_of(K), W, H, min_alpha, x0, y0, sP);
    __syncthreads();
    const int tx = threadIdx.x % DN_TILE, ty = threadIdx.x / DN_TILE;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (x > 0 && x < W - 1 && y > 0 && y < H - 1) {
        float a[3], b[3], cr[3];
        const float n2 = stencil_of<EDGE>(sP, (ty + 1) * EDGE + tx + 1, a, b, cr);
        if (n2 > 0.0f) {
            const float len = __builtin_sqrtf(n2);
            n[0] = cr[0] / len; n[1] = cr[1] / len; n[2] = cr[2] / len;
        }
    }
    float* o = normal + ((size_t)y * W + x) * 3;
    o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
}

template <bool FISH>
__global__ __launch_bounds__(NB_BLOCK) void k_depth_normal_bwd(const float* __restrict__ depth,
                                                               const float* __restrict__ alpha,
                                                               const float* __restrict__ K,
                                                               const float* __restrict__ grad_normal, int W, int H,
                                                               float min_alpha, float* __restrict__ grad_depth,
                                                               float* __restrict__ grad_alpha) {
    constexpr int EDGE = DN_TILE + 4, CEDGE = DN_TILE + 2, CCELLS = CEDGE * CEDGE;
    __shared__ float sP[3 * EDGE * EDGE];
    __shared__ float sG[6 * CCELLS];   // per centre of the tile and a halo of 1: dL/da (3 planes), dL/db (3 planes)
    const Intrinsics k = intrinsics_of(K);
    const int x0 = blockIdx.x * DN_TILE, y0 = blockIdx.y * DN_TILE;
    stage_points<FISH, 2>(depth, alpha, k, W, H, min_alpha, x0, y0, sP);
    __syncthreads();
    for (int c = threadIdx.x; c < CCELLS; c += NB_BLOCK) {
        const int cx = c % CEDGE, cy = c / CEDGE;
        const int x = x0 - 1 + cx, y = y0 - 1 + cy;
        float ga[3] = {0.0f, 0.0f, 0.0f}, gb[3] = {0.0f, 0.0f, 0.0f};
        if (x > 0 && x < W - 1 && y > 0 && y < H - 1) {
            float a[3], b[3], cr[3];
            const float n2 = stencil_of<EDGE>(sP, (cy + 1) * EDGE + cx + 1, a, b, cr);
            if (n2 > 0.0f) {
                const float len = __builtin_sqrtf(n2);
                const float n[3] = {cr[0] / len, cr[1] / len, cr[2] / len};
                const float* g = grad_normal + ((size_t)y * W + x) * 3;
                const float g0 = g[0], g1 = g[1], g2 = g[2];
                const float along = n[0] * g0 + n[1] * g1 + n[2] * g2;
                // n = cr / |cr|: dL/dcr = (g - n (n . g)) / |cr|;  cr = a x b: dL/da = b x dL/dcr, dL/db = dL/dcr x a
                const float gc[3] = {(g0 - n[0] * along) / len, (g1 - n[1] * along) / len, (g2 - n[2] * along) / len};
                ga[0] = b[1] * gc[2] - b[2] * gc[1];
                ga[1] = b[2] * gc[0] - b[0] * gc[2];
                ga[2] = b[0] * gc[1] - b[1] * gc[0];
                gb[0] = gc[1] * a[2] - gc[2] * a[1];
                gb[1] = gc[2] * a[0] - gc[0] * a[2];
                gb[2] = gc[0] * a[1] - gc[1] * a[0];
            }
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            sG[j * CCELLS + c] = ga[j];
            sG[(3 + j) * CCELLS + c] = gb[j];
        }
    }
    __syncthreads();
    const int tx = threadIdx.x % DN_TILE, ty = threadIdx.x / DN_TILE;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    float gd = 0.0f, gal = 0.0f;
    const float al = alpha[p];
    float rx, ry;
    if (al > min_alpha && ray_of<FISH>(k, x, y, rx, ry)) {
        // this pixel is P(x, y + 1) of the centre above, P(x, y - 1) of the one below, P(x + 1, y) of the one to the left
        // and P(x - 1, y) of the one to the right; in that order, always
        const int c = (ty + 1) * CEDGE + tx + 1;
        float gP[3];
#pragma unroll
        for (int j = 0; j < 3; j++)
            gP[j] = ((sG[j * CCELLS + c - CEDGE] - sG[j * CCELLS + c + CEDGE]) + sG[(3 + j) * CCELLS + c - 1]) -
                    sG[(3 + j) * CCELLS + c + 1];
        // P = d (rx, ry, 1), d = depth / alpha
        const float g_d = gP[0] * rx + gP[1] * ry + gP[2];
        const float dep = depth[p];
        gd = g_d / al;
        gal = -(g_d * dep) / (al * al);
    }
    grad_depth[p] = gd;
    grad_alpha[p] = gal;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_gaussian_normals(const void* quaternion, const void* scale, const void* camera_T_world,
                                   const int32_t* vis_idx, const void* xyz_camera_frame, int V, void* normals,
                                   void* stream) {
    GS_REQUIRE(V >= 0, "gaussian_normals: V must not be negative, got %d", V);
    if (V == 0) return GS_OK;
    GS_REQUIRE(quaternion != nullptr && scale != nullptr && camera_T_world != nullptr && vis_idx != nullptr &&
                   xyz_camera_frame != nullptr && normals != nullptr,
               "gaussian_normals: quaternion, scale, camera_T_world, vis_idx, xyz_camera_frame or normals is NULL");
    k_gaussian_normals<<<div_up(V, NB_BLOCK), NB_BLOCK, 0, (hipStream_t)stream>>>(
        (const float*)quaternion, (const float*)scale, (const float*)camera_T_world, vis_idx,
        (const float*)xyz_camera_frame, V, (float*)normals);
    return check_launch("gaussian_normals");
}

extern "C" int gs_gaussian_normals_backward(const void* quaternion, const void* scale, const void* camera_T_world,
                                            const int32_t* rank, const void* xyz_camera_frame, const void* grad_normals,
                                            int V, int N, void* grad_quaternion, void* stream) {
    GS_REQUIRE(V >= 0 && N >= 0, "gaussian_normals_backward: V and N must not be negative, got V = %d, N = %d", V, N);
    GS_REQUIRE(V <= N, "gaussian_normals_backward: V = %d visible rows of N = %d Gaussians", V, N);
    if (N == 0) return GS_OK;
    GS_REQUIRE(rank != nullptr && grad_quaternion != nullptr, "gaussian_normals_backward: rank or grad_quaternion is NULL");
    GS_REQUIRE(V == 0 || (quaternion != nullptr && scale != nullptr && camera_T_world != nullptr &&
                          xyz_camera_frame != nullptr && grad_normals != nullptr),
               "gaussian_normals_backward: quaternion, scale, camera_T_world, xyz_camera_frame or grad_normals is NULL");
    k_gaussian_normals_bwd<<<div_up(N, NB_BLOCK), NB_BLOCK, 0, (hipStream_t)stream>>>(
        (const float*)quaternion, (const float*)scale, (const float*)camera_T_world, rank, (const float*)xyz_camera_frame,
        (const float*)grad_normals, V, N, (float*)grad_quaternion);
    return check_launch("gaussian_normals_backward");
}

static int depth_normal_args(const char* who, const void* depth, const void* alpha, const void* K, const void* extra,
                             int W, int H, float min_alpha, int raster_mode, const void* out0, const void* out1) {
    GS_REQUIRE(raster_mode == GS_RASTER_CLASSIC || raster_mode == GS_RASTER_FISHEYE,
               "%s: raster_mode must be GS_RASTER_CLASSIC or GS_RASTER_FISHEYE, got %d", who, raster_mode);
    GS_REQUIRE(W >= 0 && H >= 0, "%s: W and H must not be negative, got W = %d, H = %d", who, W, H);
    GS_REQUIRE(min_alpha >= 0.0f, "%s: min_alpha must be a number >= 0, got %g", who, (double)min_alpha);
    if (W == 0 || H == 0) return GS_OK;
    GS_REQUIRE(depth != nullptr && alpha != nullptr && K != nullptr && extra != nullptr && out0 != nullptr &&
                   out1 != nullptr, "%s: a NULL pointer among the maps, K or the outputs", who);
    return GS_OK;
}

extern "C" int gs_depth_normal(const void* depth, const void* alpha, const void* K, int W, int H, float min_alpha,
                               int raster_mode, void* normal, void* stream) {
    const int rc = depth_normal_args("depth_normal", depth, alpha, K, depth, W, H, min_alpha, raster_mode, normal, normal);
    if (rc != GS_OK || W == 0 || H == 0) return rc;
    const auto kernel = raster_mode == GS_RASTER_FISHEYE ? k_depth_normal<true> : k_depth_normal<false>;
    kernel<<<dim3(div_up(W, DN_TILE), div_up(H, DN_TILE)), NB_BLOCK, 0, (hipStream_t)stream>>>(
        (const float*)depth, (const float*)alpha, (const float*)K, W, H, min_alpha, (float*)normal);
    return check_launch("depth_normal");
}

extern "C" int gs_depth_normal_backward(const void* depth, const void* alpha, const void* K, const void* grad_normal,
                                        int W, int H, float min_alpha, int raster_mode, void* grad_depth,
                                        void* grad_alpha, void* stream) {
    const int rc = depth_normal_args("depth_normal_backward", depth, alpha, K, grad_normal, W, H, min_alpha, raster_mode,
                                     grad_depth, grad_alpha);
    if (rc != GS_OK || W == 0 || H == 0) return rc;
    const auto kernel = raster_mode == GS_RASTER_FISHEYE ? k_depth_normal_bwd<true> : k_depth_normal_bwd<false>;
    kernel<<<dim3(div_up(W, DN_TILE), div_up(H, DN_TILE)), NB_BLOCK, 0, (hipStream_t)stream>>>(
        (const float*)depth, (const float*)alpha, (const float*)K, (const float*)grad_normal, W, H, min_alpha,
        (float*)grad_depth, (float*)grad_alpha);
    return check_launch("depth_normal_backward");
}
