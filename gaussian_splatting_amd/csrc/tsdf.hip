// tsdf.hip -- depth maps to a triangle mesh (include/gsplat_hip.h "TSDF fusion and mesh extraction"):
// fuse C depth maps into a truncated signed distance volume, then triangulate its level set by marching tetrahedra
// on the Kuhn split of each cell.
//
//   k_tsdf_integrate    one thread per node, lanes along x (tsdf, weight and color are coalesced).  The node's state is
//                       read once and stays in registers while the thread walks the C cameras; a camera's 16 + 9 floats
//                       are the same for every lane and come through the scalar cache (k_filter3d_rate's pattern).  The
//                       state is written back only by a thread that some view updated.  No atomics, no LDS.
//   k_tsdf_active       one thread per cell: are all 8 corners observed (weight >= min_weight)?  A byte per node.
//   k_tsdf_count        one thread per node: the 7-bit mask of its owned edges that carry a vertex, its popcount, and
//                       the number of triangles of the node's cell.  The caller scans the two counts.
//   k_tsdf_emit_vertices / k_tsdf_emit_faces
//                       one thread per node: the vertices of its owned edges at offset[n] + rank; the triangles of its
//                       cell, a vertex id being offset[owner] + popcount(mask[owner] & ((1 << e) - 1)).
//
// All kernels map threads to nodes the same way: a 64 x 4 block covers 64 nodes along x of 4 rows (j); blockIdx.z = k.
// The projection is the per-Gaussian stage's own (pg_math.h: to_camera, then the pinhole expression of is_culled or
// fisheye_project), so a node falls on the pixel where a Gaussian at its position would be drawn.
#include "pg_math.h"

namespace gs {

constexpr int TS_BX = 64, TS_BY = 4;
constexpr int TS_MAX_ROWS = 65535;   // gridDim.y and gridDim.z

struct TsdfDims {
    int nx, ny, nz;
};

__device__ inline bool node_of_thread(const TsdfDims& D, int& i, int& j, int& k) {
    i = blockIdx.x * TS_BX + threadIdx.x;
    j = blockIdx.y * TS_BY + threadIdx.y;
    k = blockIdx.z;
    return i < D.nx && j < D.ny;
}
__device__ inline int64_t node_index(const TsdfDims& D, int i, int j, int k) {
    return ((int64_t)k * D.ny + j) * D.nx + i;
}
static dim3 tsdf_grid(int nx, int ny, int nz) { return dim3(div_up(nx, TS_BX), div_up(ny, TS_BY), nz); }

// ---- integration ------------------------------------------------------------------------------------------------------
template <bool FISH, bool COLOR>
__global__ __launch_bounds__(TS_BX* TS_BY) void k_tsdf_integrate(
    const float* __restrict__ depth /* [C,H,W] */, const float* __restrict__ image /* [C,H,W,3] */,
    const float* __restrict__ cams /* [C,4,4] */, const float* __restrict__ Ks /* [C,3,3] */, int C, int W, int H, float near,
    float trunc, float max_weight, float depth_max, float ox, float oy, float oz, float voxel, TsdfDims D,
    float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color) {
    int i, j, k;
    if (!node_of_thread(D, i, j, k)) return;
    const int64_t n = node_index(D, i, j, k);
    const float px = ox + voxel * (float)i, py = oy + voxel * (float)j, pz = oz + voxel * (float)k;
    float t_acc = tsdf[n], w_acc = weight[n];
    float r_acc = 0.0f, g_acc = 0.0f, b_acc = 0.0f;
    if constexpr (COLOR) {
        r_acc = color[n * 3 + 0];
        g_acc = color[n * 3 + 1];
        b_acc = color[n * 3 + 2];
    }
    bool touched = false;
    const float fw = (float)W, fh = (float)H;
    for (int v = 0; v < C; v++) {
        const float* M = cams + (size_t)v * 16;
        const float* K = Ks + (size_t)v * 9;
        float c[3], uv[2];
        to_camera(M, px, py, pz, c);
        if (!(c[2] > near)) continue;
        if constexpr (FISH) {
            fisheye_project(c, fisheye_terms_of(c), K[0], K[4], K[2], K[5], uv);
        } else {
            uv[0] = K[0] * c[0] / c[2] + K[2];   // (is_culled's expression)
            uv[1] = K[4] * c[1] / c[2] + K[5];
        }
        const float fu = __builtin_floorf(uv[0] + 0.5f), fv = __builtin_floorf(uv[1] + 0.5f);
        if (!(fu >= 0.0f && fu < fw && fv >= 0.0f && fv < fh)) continue;   // a NaN compares false
        const size_t pix = ((size_t)v * H + (int)fv) * W + (int)fu;
        const float d = depth[pix];
        if (!(d > 0.0f && d <= depth_max && d < __builtin_inff())) continue;
        const float dist = __builtin_sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const float sdf = (d - c[2]) * (dist / c[2]);
        if (!(sdf >= -trunc)) continue;
        const float t = fminf(1.0f, sdf / trunc);
        const float w1 = w_acc + 1.0f;
        t_acc = (t_acc * w_acc + t) / w1;
        if constexpr (COLOR) {
            r_acc = (r_acc * w_acc + image[pix * 3 + 0]) / w1;
            g_acc = (g_acc * w_acc + image[pix * 3 + 1]) / w1;
            b_acc = (b_acc * w_acc + image[pix * 3 + 2]) / w1;
        }
        w_acc = fminf(w1, max_weight);
        touched = true;
    }
    if (!touched) return;
    tsdf[n] = t_acc;
    weight[n] = w_acc;
    if constexpr (COLOR) {
        color[n * 3 + 0] = r_acc;
        color[n * 3 + 1] = g_acc;
        color[n * 3 + 2] = b_acc;
    }
}

// ---- extraction -------------------------------------------------------------------------------------------------------
// Corners and directions are 3-bit masks, x = 1, y = 2, z = 4.  Edge direction e = 0..6 has the mask DIR_MASK[e].
__device__ constexpr int DIR_MASK[7] = {1, 2, 4, 3, 5, 6, 7};
__device__ __host__ constexpr int dir_of_mask(int m) { return m == 1 ? 0 : m == 2 ? 1 : m == 4 ? 2 : m == 3 ? 3 : m == 5 ? 4 : m == 6 ? 5 : 6; }
// Tetrahedron q = {000, e_a, e_a + e_b, 111}, (a, b, c) = xyz, xzy, yxz, yzx, zxy, zyx: the corner masks of v1 and v2, and
// whether (v0, v1, v2, v3) is a left-handed frame (an odd permutation of the axes).
__device__ constexpr int TET_V1[6] = {1, 1, 2, 2, 4, 4};
__device__ constexpr int TET_V2[6] = {3, 5, 3, 6, 5, 6};
__device__ constexpr bool TET_ODD[6] = {false, true, true, false, false, true};
// The triangles of a right-handed tetrahedron by its inside mask m (bit i: corner v_i has f < 0).  Tetrahedron edges
// 0..5 = v0v1, v0v2, v0v3, v1v2, v1v3, v2v3.  Bits 0-1: the number of triangles; bits 2-10 and 11-19: three edge numbers
// of 3 bits each.  One inside corner p (or one outside): the edges from p to the other corners in ascending order,
// reversed when p is odd (when p is even); two inside p < q, outside r < s: the quad pr, ps, qs, qr split along pr - qs,
// reversed when p + q is even.  A left-handed tetrahedron swaps the last two corners of every triangle.
// (tests/mesh_ref.py derives the same windings from the geometry instead.)
__device__ constexpr unsigned TET_CASES[16] = {0x0u,     0x221u,   0x381u,   0x70c46u, 0x565u,   0xac2a2u, 0x34582u, 0x589u,
                                               0x4a9u,   0x94522u, 0xa83a2u, 0x3a5u,   0x50c66u, 0x461u,   0x141u,   0x0u};

__device__ inline int tet_triangles(int m) { return (0x01210u >> (__builtin_popcount(m) * 4)) & 0xfu; }   // 0 1 2 1 0 triangles for 0..4 inside

__global__ __launch_bounds__(TS_BX* TS_BY) void k_tsdf_active(const float* __restrict__ weight, TsdfDims D, float min_weight,
                                                              uint8_t* __restrict__ active) {
    int i, j, k;
    if (!node_of_thread(D, i, j, k)) return;
    const int64_t n = node_index(D, i, j, k);
    bool a = i + 1 < D.nx && j + 1 < D.ny && k + 1 < D.nz;
    if (a) {
#pragma unroll
        for (int o = 0; o < 8; o++) {
            const int64_t m = node_index(D, i + (o & 1), j + ((o >> 1) & 1), k + (o >> 2));
            a = a && weight[m] >= min_weight;
        }
    }
    active[n] = a ? 1 : 0;
}

__global__ __launch_bounds__(TS_BX* TS_BY) void k_tsdf_count(const float* __restrict__ tsdf, const uint8_t* __restrict__ active,
                                                             TsdfDims D, float level, uint8_t* __restrict__ edge_mask,
                                                             int* __restrict__ vert_count, int* __restrict__ face_count) {
    int i, j, k;
    if (!node_of_thread(D, i, j, k)) return;
    const int64_t n = node_index(D, i, j, k);
    // act bit o: the cell whose corner o this node is (low corner = node - o) is active
    unsigned act = 0;
#pragma unroll
    for (int o = 0; o < 7; o++) {
        const int ci = i - (o & 1), cj = j - ((o >> 1) & 1), ck = k - (o >> 2);
        if (ci >= 0 && cj >= 0 && ck >= 0 && active[node_index(D, ci, cj, ck)]) act |= 1u << o;
    }
    int mask = 0, faces = 0;
    if (act) {
        // inside bit c: corner c of this node's cell has f < 0 (corners outside the volume: never read, never used)
        unsigned inside = 0, there = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int bi = i + (c & 1), bj = j + ((c >> 1) & 1), bk = k + (c >> 2);
            if (bi < D.nx && bj < D.ny && bk < D.nz) {
                there |= 1u << c;
                if (tsdf[node_index(D, bi, bj, bk)] - level < 0.0f) inside |= 1u << c;
            }
        }
        const unsigned differs = (inside ^ (0u - (inside & 1u))) & there;   // corner c differs in sign from this node
#pragma unroll
        for (int e = 0; e < 7; e++) {
            const int d = DIR_MASK[e];
            unsigned owners = 0;   // the corners o of a cell from which direction d stays inside the cell: o & d == 0
#pragma unroll
            for (int o = 0; o < 7; o++)
                if ((o & d) == 0) owners |= 1u << o;
            if ((differs >> d & 1u) && (act & owners)) mask |= 1 << e;
        }
        if (act & 1u) {
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const int m = (inside & 1u) | ((inside >> TET_V1[q] & 1u) << 1) | ((inside >> TET_V2[q] & 1u) << 2) |
                              ((inside >> 7 & 1u) << 3);
                faces += tet_triangles(m);
            }
        }
    }
    edge_mask[n] = (uint8_t)mask;
    vert_count[n] = __builtin_popcount(mask);
    face_count[n] = faces;
}

template <bool COLOR>
__global__ __launch_bounds__(TS_BX* TS_BY) void k_tsdf_emit_vertices(const float* __restrict__ tsdf, const float* __restrict__ color,
                                                                     const uint8_t* __restrict__ edge_mask,
                                                                     const int* __restrict__ vert_offset, TsdfDims D, float level,
                                                                     float ox, float oy, float oz, float voxel,
                                                                     float* __restrict__ vertices, float* __restrict__ colors) {
    int i, j, k;
    if (!node_of_thread(D, i, j, k)) return;
    const int64_t n = node_index(D, i, j, k);
    const int mask = edge_mask[n];
    if (!mask) return;
    int64_t out = vert_offset[n];
    const float fa = tsdf[n] - level;
    float ca[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (COLOR) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) ca[ch] = color[n * 3 + ch];
    }
#pragma unroll
    for (int e = 0; e < 7; e++) {
        if (!(mask >> e & 1)) continue;
        const int d = DIR_MASK[e];
        const int64_t b = node_index(D, i + (d & 1), j + ((d >> 1) & 1), k + (d >> 2));
        const float fb = tsdf[b] - level;
        const float s = fa / (fa - fb);
        vertices[out * 3 + 0] = ox + voxel * ((float)i + s * (float)(d & 1));
        vertices[out * 3 + 1] = oy + voxel * ((float)j + s * (float)((d >> 1) & 1));
        vertices[out * 3 + 2] = oz + voxel * ((float)k + s * (float)(d >> 2));
        if constexpr (COLOR) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) colors[out * 3 + ch] = ca[ch] + s * (color[b * 3 + ch] - ca[ch]);
        }
        out++;
    }
}

__device__ inline int pick6(int idx, int e0, int e1, int e2, int e3, int e4, int e5) {
    return idx == 0 ? e0 : idx == 1 ? e1 : idx == 2 ? e2 : idx == 3 ? e3 : idx == 4 ? e4 : e5;
}

__global__ __launch_bounds__(TS_BX* TS_BY) void k_tsdf_emit_faces(const float* __restrict__ tsdf, const uint8_t* __restrict__ edge_mask,
                                                                  const int* __restrict__ vert_offset,
                                                                  const int* __restrict__ face_offset,
                                                                  const int* __restrict__ face_count, TsdfDims D, float level,
                                                                  int* __restrict__ faces) {
    int i, j, k;
    if (!node_of_thread(D, i, j, k)) return;
    const int64_t n = node_index(D, i, j, k);
    if (face_count[n] <= 0) return;   // an inactive cell, a cell without a crossing, or no cell at all
    unsigned inside = 0;
    int voff[7], vmask[7];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const int64_t m = node_index(D, i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2));
        if (tsdf[m] - level < 0.0f) inside |= 1u << c;
        if (c < 7) {   // corner 7 owns no edge of this cell
            voff[c] = vert_offset[m];
            vmask[c] = edge_mask[m];
        }
    }
    int64_t out = face_offset[n];
#pragma unroll
    for (int q = 0; q < 6; q++) {
        const int corner[4] = {0, TET_V1[q], TET_V2[q], 7};
        const int m = (inside & 1u) | ((inside >> corner[1] & 1u) << 1) | ((inside >> corner[2] & 1u) << 2) |
                      ((inside >> 7 & 1u) << 3);
        const unsigned entry = TET_CASES[m];
        const int count = entry & 3u;
        if (count == 0) continue;
        // the vertex of tetrahedron edge v_a v_b: owned by corner[a], direction corner[b] - corner[a]
        int ev[6];
        int t = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = a + 1; b < 4; b++) {
                const int e = dir_of_mask(corner[b] ^ corner[a]);
                ev[t++] = voff[corner[a]] + __builtin_popcount(vmask[corner[a]] & ((1 << e) - 1));
            }
        }
        for (int tri = 0; tri < count; tri++) {
            const unsigned w = entry >> (2 + 9 * tri);
            const int v0 = pick6(w & 7u, ev[0], ev[1], ev[2], ev[3], ev[4], ev[5]);
            const int v1 = pick6(w >> 3 & 7u, ev[0], ev[1], ev[2], ev[3], ev[4], ev[5]);
            const int v2 = pick6(w >> 6 & 7u, ev[0], ev[1], ev[2], ev[3], ev[4], ev[5]);
            faces[out * 3 + 0] = v0;
            faces[out * 3 + 1] = TET_ODD[q] ? v2 : v1;
            faces[out * 3 + 2] = TET_ODD[q] ? v1 : v2;
            out++;
        }
    }
}

static bool tsdf_dims_ok(int nx, int ny, int nz) { return nx >= 0 && ny >= 0 && nz >= 0 && ny <= TS_MAX_ROWS * TS_BY && nz <= TS_MAX_ROWS; }

}  // namespace gs

using namespace gs;

#define TSDF_DIMS_MSG "%s: nx, ny, nz must not be negative, ny <= 262140 and nz <= 65535, got %d x %d x %d"

extern "C" int gs_tsdf_integrate(const void* depth, const void* image, const void* camera_T_world, const void* K, int C, int W,
                                 int H, int raster_mode, float near_thresh, float sdf_trunc, float max_weight, float depth_max,
                                 float origin_x, float origin_y, float origin_z, float voxel_size, int nx, int ny, int nz,
                                 void* tsdf, void* weight, void* color, void* stream) {
    GS_REQUIRE(raster_mode == GS_RASTER_CLASSIC || raster_mode == GS_RASTER_FISHEYE,
               "tsdf_integrate: raster_mode must be GS_RASTER_CLASSIC or GS_RASTER_FISHEYE, got %d", raster_mode);
    GS_REQUIRE(C >= 0 && W >= 0 && H >= 0, "tsdf_integrate: C, W and H must not be negative, got C = %d, W = %d, H = %d", C, W, H);
    GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), TSDF_DIMS_MSG, "tsdf_integrate", nx, ny, nz);
    GS_REQUIRE(sdf_trunc > 0.0f && sdf_trunc < __builtin_inff() && max_weight > 0.0f,
               "tsdf_integrate: sdf_trunc must be finite and > 0 and max_weight > 0, got %g and %g", (double)sdf_trunc,
               (double)max_weight);
    GS_REQUIRE(near_thresh == near_thresh && depth_max == depth_max && voxel_size == voxel_size && origin_x == origin_x &&
                   origin_y == origin_y && origin_z == origin_z,
               "tsdf_integrate: near_thresh, depth_max, voxel_size or origin is not a number");
    GS_REQUIRE((image == nullptr) == (color == nullptr),
               "tsdf_integrate: image and color go together: give both (a coloured volume) or neither");
    if (C == 0 || W == 0 || H == 0 || nx == 0 || ny == 0 || nz == 0) return GS_OK;
    GS_REQUIRE(depth != nullptr && camera_T_world != nullptr && K != nullptr && tsdf != nullptr && weight != nullptr,
               "tsdf_integrate: depth, camera_T_world, K, tsdf or weight is NULL");
    const bool fish = raster_mode == GS_RASTER_FISHEYE;
    const auto kernel = color ? (fish ? k_tsdf_integrate<true, true> : k_tsdf_integrate<false, true>)
                              : (fish ? k_tsdf_integrate<true, false> : k_tsdf_integrate<false, false>);
    kernel<<<tsdf_grid(nx, ny, nz), dim3(TS_BX, TS_BY), 0, (hipStream_t)stream>>>(
        (const float*)depth, (const float*)image, (const float*)camera_T_world, (const float*)K, C, W, H, near_thresh, sdf_trunc,
        max_weight, depth_max, origin_x, origin_y, origin_z, voxel_size, TsdfDims{nx, ny, nz}, (float*)tsdf, (float*)weight,
        (float*)color);
    return check_launch("tsdf_integrate");
}

extern "C" size_t gs_tsdf_extract_workspace_bytes(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    return (size_t)nx * (size_t)ny * (size_t)nz;
}

extern "C" int gs_tsdf_extract_count(const void* tsdf, const void* weight, int nx, int ny, int nz, float level, float min_weight,
                                     void* workspace, void* edge_mask, int32_t* vert_count, int32_t* face_count, void* stream) {
    GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), TSDF_DIMS_MSG, "tsdf_extract_count", nx, ny, nz);
    GS_REQUIRE(min_weight > 0.0f && level == level, "tsdf_extract_count: min_weight must be > 0 and level a number, got %g and %g",
               (double)min_weight, (double)level);
    if (nx == 0 || ny == 0 || nz == 0) return GS_OK;
    GS_REQUIRE(tsdf != nullptr && weight != nullptr && workspace != nullptr && edge_mask != nullptr && vert_count != nullptr &&
                   face_count != nullptr,
               "tsdf_extract_count: tsdf, weight, workspace, edge_mask, vert_count or face_count is NULL");
    const TsdfDims D{nx, ny, nz};
    const dim3 grid = tsdf_grid(nx, ny, nz), block(TS_BX, TS_BY);
    k_tsdf_active<<<grid, block, 0, (hipStream_t)stream>>>((const float*)weight, D, min_weight, (uint8_t*)workspace);
    k_tsdf_count<<<grid, block, 0, (hipStream_t)stream>>>((const float*)tsdf, (const uint8_t*)workspace, D, level,
                                                          (uint8_t*)edge_mask, vert_count, face_count);
    return check_launch("tsdf_extract_count");
}

extern "C" int gs_tsdf_extract_emit(const void* tsdf, const void* color, const void* edge_mask, const int32_t* vert_offset,
                                    const int32_t* face_offset, const int32_t* face_count, int nx, int ny, int nz, float level,
                                    float origin_x, float origin_y, float origin_z, float voxel_size, void* vertices, void* colors,
                                    int32_t* faces, void* stream) {
    GS_REQUIRE(tsdf_dims_ok(nx, ny, nz), TSDF_DIMS_MSG, "tsdf_extract_emit", nx, ny, nz);
    GS_REQUIRE(level == level && voxel_size == voxel_size && origin_x == origin_x && origin_y == origin_y && origin_z == origin_z,
               "tsdf_extract_emit: level, voxel_size or origin is not a number");
    GS_REQUIRE((color == nullptr) == (colors == nullptr),
               "tsdf_extract_emit: color and colors go together: give both (a coloured volume) or neither");
    if (nx == 0 || ny == 0 || nz == 0) return GS_OK;
    GS_REQUIRE(tsdf != nullptr && edge_mask != nullptr && vert_offset != nullptr && face_offset != nullptr &&
                   face_count != nullptr && vertices != nullptr && faces != nullptr,
               "tsdf_extract_emit: tsdf, edge_mask, vert_offset, face_offset, face_count, vertices or faces is NULL");
    const TsdfDims D{nx, ny, nz};
    const dim3 grid = tsdf_grid(nx, ny, nz), block(TS_BX, TS_BY);
    const auto kernel = color ? k_tsdf_emit_vertices<true> : k_tsdf_emit_vertices<false>;
    kernel<<<grid, block, 0, (hipStream_t)stream>>>((const float*)tsdf, (const float*)color, (const uint8_t*)edge_mask, vert_offset, D,
                                                    level, origin_x, origin_y, origin_z, voxel_size, (float*)vertices,
                                                    (float*)colors);
    k_tsdf_emit_faces<<<grid, block, 0, (hipStream_t)stream>>>((const float*)tsdf, (const uint8_t*)edge_mask, vert_offset, face_offset,
                                                               face_count, D, level, faces);
    return check_launch("tsdf_extract_emit");
}
