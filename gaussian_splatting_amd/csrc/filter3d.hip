// filter3d.hip -- the sampling rate behind the 3D smoothing filter (include/gsplat_hip.h "3D smoothing filter",
// DESIGN.md 7k): for every Gaussian the finest rate, in pixels per world unit, at which any of C cameras samples it.
//
//   k_filter3d_rate   one thread per Gaussian: its position is read once and stays in registers while the thread walks
//                     the C cameras.  A camera's 16 + 9 floats and 2 ints are the same for every lane, so the compiler
//                     fetches them through the scalar cache; per camera a thread spends ~25 VALU instructions (pinhole).
//                     rate[g] is read, raised and written back only when a camera raised it.
//
// The projection is the per-Gaussian stage's own (pg_math.h: to_camera, then the pinhole expression of is_culled or
// fisheye_project), so a Gaussian is "in view" here exactly where the frame's uv would say so.
#include "pg_math.h"

namespace gs {

constexpr int F3_BLOCK = 256;

template <bool FISH>
__global__ __launch_bounds__(F3_BLOCK) void k_filter3d_rate(const float* __restrict__ xyz,
                                                            const float* __restrict__ cams /* [C,4,4] */,
                                                            const float* __restrict__ Ks /* [C,3,3] */,
                                                            const int* __restrict__ sizes /* [C,2] */, int C, int N,
                                                            float near, float pad, float* __restrict__ rate) {
    const int g = blockIdx.x * F3_BLOCK + threadIdx.x;
    if (g >= N) return;
    const float px = xyz[(size_t)g * 3 + 0], py = xyz[(size_t)g * 3 + 1], pz = xyz[(size_t)g * 3 + 2];
    const float before = rate[g];
    float best = before;
    for (int k = 0; k < C; k++) {
        const float* M = cams + (size_t)k * 16;
        const float* K = Ks + (size_t)k * 9;
        const float w = (float)sizes[2 * k + 0], h = (float)sizes[2 * k + 1];
        const float fx = K[0], fy = K[4];
        float c[3], uv[2], dist;
        to_camera(M, px, py, pz, c);
        if constexpr (FISH) {
            fisheye_project(c, fisheye_terms_of(c), fx, fy, K[2], K[5], uv);
            dist = __builtin_sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        } else {
            uv[0] = fx * c[0] / c[2] + K[2];   // (is_culled's expression)
            uv[1] = fy * c[1] / c[2] + K[5];
            dist = c[2];
        }
        const float pu = pad * w, pv = pad * h;
        const bool in_view = (c[2] > near) & (uv[0] > -pu) & (uv[0] < w + pu) & (uv[1] > -pv) & (uv[1] < h + pv);
        const float r = fmaxf(fx, fy) / dist;
        if (in_view && r > best) best = r;
    }
    if (best > before) rate[g] = best;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_filter3d_rate(const void* xyz, const void* camera_T_world, const void* K, const int32_t* sizes, int C,
                                int N, float near_thresh, float pad_fraction, int raster_mode, void* rate, void* stream) {
    GS_REQUIRE(raster_mode == GS_RASTER_CLASSIC || raster_mode == GS_RASTER_FISHEYE,
               "filter3d_rate: raster_mode must be GS_RASTER_CLASSIC or GS_RASTER_FISHEYE, got %d", raster_mode);
    GS_REQUIRE(C >= 0 && N >= 0, "filter3d_rate: C and N must not be negative, got C = %d, N = %d", C, N);
    if (C == 0 || N == 0) return GS_OK;
    GS_REQUIRE(xyz != nullptr && camera_T_world != nullptr && K != nullptr && sizes != nullptr && rate != nullptr,
               "filter3d_rate: xyz, camera_T_world, K, sizes or rate is NULL");
    const auto kernel = raster_mode == GS_RASTER_FISHEYE ? k_filter3d_rate<true> : k_filter3d_rate<false>;
    kernel<<<div_up(N, F3_BLOCK), F3_BLOCK, 0, (hipStream_t)stream>>>((const float*)xyz, (const float*)camera_T_world,
                                                                      (const float*)K, sizes, C, N, near_thresh,
                                                                      pad_fraction, (float*)rate);
    return check_launch("filter3d_rate");
}
