// bilagrid.hip -- per-image bilateral grids of affine colour transforms between the rendered image and the loss
// ("Bilateral Guided Radiance Field Processing").  No reference counterpart.
//
//   grid  [12, L, Hg, Wg]   channel 4r + j is entry (r, j) of a 3x4 affine A
//   image [H, W, 3]         the rasterizer's layout
//
// Pixel (px, py) samples the grid at gx = (px + 0.5) / W (Wg - 1), gy likewise, gz = clamp(luma, 0, 1) (L - 1),
// trilinearly (border clamp, align_corners), and out = A(p) (R, G, B, 1).  The xy cell of a pixel is an INTEGER
// function of its column / row (bg_cell), so the kernels, the host and the tests can never disagree on it, and the
// fraction is one correctly rounded division of two exact integers.  Every axis interpolates in the lerp form
// a0 + f (a1 - a0): equal corners give their common value exactly, so an identity grid returns the image's bits.
//
//   k_bilagrid_slice        64x16 pixel tile per workgroup, four pixels of a row per lane (three 16-byte accesses);
//                           the nodes the tile touches are staged in LDS, node-major (12 consecutive floats per node)
//   k_bilagrid_slice_bwd    one workgroup per chunk of <= 1024 pixels of ONE xy cell (all of them share four xy
//                           nodes): grad_image is a gather; grad_grid is summed per z node in 48 registers per lane,
//                           across lanes by a halving butterfly, across the four waves in wave order, and written as
//                           the chunk's 4 L 12 partials
//   k_bilagrid_grad_finish  every grid element sums the partials of the <= 4 cells around its node, chunks in index
//                           order: no atomics anywhere, the same bits on every call, unreached nodes exact zeros
//   k_bilagrid_tv (+finish) total variation of a stack of grids: fp64 per-workgroup partials reduced in a fixed
//                           order (the pattern of k_ssim_l1 / k_loss_finish); the gradient is a six-neighbour gather
#include "gs_common.h"

namespace gs {

constexpr int BG_THREADS = 256;
constexpr int BG_PPL = 4;                         // pixels per lane
constexpr int BG_TX = 16 * BG_PPL, BG_TY = 16;    // forward tile: 64 x 16 pixels
constexpr int BG_CHUNK = BG_THREADS * BG_PPL;     // backward: pixels of one cell per workgroup
constexpr int BG_FWD_LDS = 4096;                  // floats of staged nodes (16 KiB); larger boxes read the grid in place
constexpr int BG_TV_PER = 16;                     // total variation: elements per lane
constexpr int BG_BWD_LMAX = 64;                   // deepest grid the backward stages (4 L 12 floats = 12 KiB)

struct BgDims {
    int H, W, L, Hg, Wg;
};

// cell of pixel column (row) p on an axis of n nodes over N pixels: floor((p + 0.5) / N (n - 1)) in integers
__host__ __device__ inline int bg_cell(int p, int n, int N) {
    if (n < 2) return 0;
    const int c = (int)((2u * (unsigned)p + 1u) * (unsigned)(n - 1) / (2u * (unsigned)N));   // N n < 2^30 (BG_REQUIRE_DIMS)
    return c < n - 2 ? c : n - 2;
}
// first pixel whose cell is >= c (N for c past the last cell): cell c owns [bg_cell_start(c), bg_cell_start(c + 1))
__host__ __device__ inline int bg_cell_start(int c, int n, int N) {
    if (c <= 0) return 0;
    if (n < 2 || c >= n - 1) return N;
    const int num = 2 * N * c - (n - 1), den = 2 * (n - 1);
    return num <= 0 ? 0 : (int)(((unsigned)num + (unsigned)den - 1u) / (unsigned)den);
}
// g - i0 for the pixel's own cell: both integers are exact in fp32 (N < 2^23), so this is one rounding
__device__ inline float bg_frac(int p, int c, int n, int N) {
    if (n < 2) return 0.0f;
    const int rem = (2 * p + 1) * (n - 1) - 2 * N * c;
    return (float)rem / (float)(2 * N);
}
// upper bound of the nodes that `span` consecutive pixels touch on an axis
inline int bg_nodes_bound(int span, int n, int N) {
    if (n < 2) return 1;
    const int64_t b = ((int64_t)span * (n - 1)) / N + 3;
    return b < n ? (int)b : n;
}

// the guidance axis.  open: the border clamp's derivative is 1 (PyTorch's definition: strictly inside)
__device__ inline void bg_z(float r, float g, float b, int L, int& z0, int& z1, float& fz, bool& open) {
    const float lum = (0.299f * r + 0.587f * g) + 0.114f * b;
    open = lum > 0.0f && lum < 1.0f && L > 1;
    const float gz = fminf(fmaxf(lum, 0.0f), 1.0f) * (float)(L - 1);   // NaN -> 0: the indices stay inside
    const int i = (int)gz, top = L > 2 ? L - 2 : 0;
    z0 = i < top ? i : top;
    z1 = z0 + 1 < L ? z0 + 1 : L - 1;
    fz = gz - (float)z0;
}

// A = trilinear sample of the 12 channels, dA = dA / dgz (the z-lerp's a1 - a0, interpolated in x and y).
// g points at node (x0, y0, z = 0) of the pixel's cell; cs / zs: channel and z strides; xs / ys: distance to the
// cell's x1 / y1 node (0 on an axis of one node)
template <bool DERIV>
__device__ inline void bg_interp(const float* g, int cs, int xs, int ys, int zs, int z0, int z1, float fx, float fy,
                                 float fz, float* A, float* dA) {
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const float* p0 = g + k * cs + z0 * zs;
        const float* p1 = g + k * cs + z1 * zs;
        const float a00 = p0[0], a01 = p0[xs], a10 = p0[ys], a11 = p0[ys + xs];
        const float b00 = p1[0], b01 = p1[xs], b10 = p1[ys], b11 = p1[ys + xs];
        const float a0 = a00 + fx * (a01 - a00), a1 = a10 + fx * (a11 - a10);
        const float b0 = b00 + fx * (b01 - b00), b1 = b10 + fx * (b11 - b10);
        const float lo = a0 + fy * (a1 - a0), hi = b0 + fy * (b1 - b0);
        const float d = hi - lo;
        A[k] = lo + fz * d;
        if (DERIV) dA[k] = d;
    }
}

// 16 bytes at 4-byte alignment: gfx950 takes a misaligned global dwordx4, so rows of any width keep wide accesses
typedef float bg_f2 __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(4))) bg_f4 {
    float v[4];
};

// stage the box of nodes [cx_lo, cx_lo + nx) x [cy_lo, cy_lo + ny) x [0, L) node-major: s[node * 12 + k]
__device__ inline void bg_stage(float* s, int cap, const float* __restrict__ grid, const BgDims& D, int cx_lo, int nx,
                                int cy_lo, int ny) {
    const int nodes = nx * ny * D.L;
    const int n = nodes * 12 < cap ? nodes * 12 : cap;
    for (int idx = threadIdx.x; idx < n; idx += BG_THREADS) {
        const int k = idx / nodes, node = idx - k * nodes;
        const int xl = node % nx, yl = (node / nx) % ny, z = node / (nx * ny);
        s[node * 12 + k] = grid[(((size_t)k * D.L + z) * D.Hg + cy_lo + yl) * D.Wg + cx_lo + xl];
    }
    __syncthreads();
}

template <bool STAGED>
__global__ __launch_bounds__(BG_THREADS) void k_bilagrid_slice(const float* __restrict__ grid,
                                                               const float* __restrict__ img, BgDims D,
                                                               float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_g[STAGED ? BG_FWD_LDS : 4];
    const int tx0 = blockIdx.x * BG_TX, ty0 = blockIdx.y * BG_TY;
    const int tx1 = min(tx0 + BG_TX, D.W) - 1, ty1 = min(ty0 + BG_TY, D.H) - 1;
    const int cx_lo = bg_cell(tx0, D.Wg, D.W), cy_lo = bg_cell(ty0, D.Hg, D.H);
    const int nx = D.Wg < 2 ? 1 : bg_cell(tx1, D.Wg, D.W) - cx_lo + 2;
    const int ny = D.Hg < 2 ? 1 : bg_cell(ty1, D.Hg, D.H) - cy_lo + 2;
    // the lane's pixels are requested before the nodes are staged: the two latencies overlap
    const int py = ty0 + (int)threadIdx.x / 16, px0 = tx0 + ((int)threadIdx.x % 16) * BG_PPL;
    const bool active = py < D.H && px0 < D.W;
    const size_t o = ((size_t)py * D.W + px0) * 3;
    const bool full = px0 + BG_PPL <= D.W;
    float v[3 * BG_PPL];
    if (active && full) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const bg_f4 t = *reinterpret_cast<const bg_f4*>(img + o + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; i++) v[4 * q + i] = t.v[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3 * BG_PPL; i++) v[i] = active && px0 + i / 3 < D.W ? img[o + i] : 0.0f;
    }
    if (STAGED) bg_stage(s_g, BG_FWD_LDS, grid, D, cx_lo, nx, cy_lo, ny);
    if (!active) return;
    const int cy = bg_cell(py, D.Hg, D.H);
    const float fy = bg_frac(py, cy, D.Hg, D.H);
    const int one_x = D.Wg > 1, one_y = D.Hg > 1;
    // A real loop, one pixel's 96 node reads in flight at a time (unrolled, the four pixels' reads are all issued
    // first and cost 300 registers).  v rotates by one pixel per trip: the trip reads the front, appends its result,
    // and after BG_PPL trips v holds the outputs in order without ever being indexed by the loop counter.
#pragma unroll 1
    for (int i = 0; i < BG_PPL; i++) {
        const int px = min(px0 + i, D.W - 1);
        const int cx = bg_cell(px, D.Wg, D.W);
        const float fx = bg_frac(px, cx, D.Wg, D.W);
        const float R = v[0], G = v[1], B = v[2];
        int z0, z1;
        float fz;
        bool open;
        bg_z(R, G, B, D.L, z0, z1, fz, open);
        float A[12];
        if (STAGED)
            bg_interp<false>(s_g + ((cy - cy_lo) * nx + (cx - cx_lo)) * 12, 1, one_x * 12, one_y * nx * 12,
                             nx * ny * 12, z0, z1, fx, fy, fz, A, nullptr);
        else
            bg_interp<false>(grid + (size_t)cy * D.Wg + cx, D.L * D.Hg * D.Wg, one_x, one_y * D.Wg, D.Hg * D.Wg, z0,
                             z1, fx, fy, fz, A, nullptr);
#pragma unroll
        for (int q = 0; q < 3 * (BG_PPL - 1); q++) v[q] = v[q + 3];
#pragma unroll
        for (int r = 0; r < 3; r++)
            v[3 * (BG_PPL - 1) + r] = ((A[4 * r] * R + A[4 * r + 1] * G) + A[4 * r + 2] * B) + A[4 * r + 3];
    }
    if (full) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            bg_f4 t;
#pragma unroll
            for (int i = 0; i < 4; i++) t.v[i] = v[4 * q + i];
            *reinterpret_cast<bg_f4*>(out + o + 4 * q) = t;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3 * BG_PPL; i++)
            if (px0 + i / 3 < D.W) out[o + i] = v[i];
    }
}

// one step of the halving butterfly: the lane whose bit `m` is clear keeps the sums of the first N / 2 values, its
// partner those of the second half.  Every sum is formed by exactly one lane from the same two operands.
template <int N>
__device__ inline void bg_halve(float* a, int m) {
    const bool up = (threadIdx.x & m) != 0;
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
        const float keep = up ? a[N / 2 + i] : a[i], send = up ? a[i] : a[N / 2 + i];
        a[i] = keep + __shfl_xor(send, m);
    }
}

// a lane's per-pixel arrays, rotated by one pixel
template <typename T>
__device__ inline void bg_rotate1(T (&a)[BG_PPL]) {
    const T t = a[0];
#pragma unroll
    for (int j = 0; j + 1 < BG_PPL; j++) a[j] = a[j + 1];
    a[BG_PPL - 1] = t;
}
__device__ inline void bg_rotate3(float (&a)[BG_PPL][3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float t = a[0][c];
#pragma unroll
        for (int j = 0; j + 1 < BG_PPL; j++) a[j][c] = a[j + 1][c];
        a[BG_PPL - 1][c] = t;
    }
}

template <bool STAGED>
__global__ __launch_bounds__(BG_THREADS) void k_bilagrid_slice_bwd(const float* __restrict__ grid,
                                                                   const float* __restrict__ img,
                                                                   const float* __restrict__ gout, BgDims D, int ncx,
                                                                   int nchunk, float* __restrict__ ws,
                                                                   float* __restrict__ gimg) {
    __shared__ __attribute__((aligned(16))) float s_g[STAGED ? 4 * BG_BWD_LMAX * 12 : 4];
    __shared__ float s_red[BG_THREADS / GS_WAVE][48];
    const int tid = threadIdx.x;
    const int cell = blockIdx.x / nchunk, chunk = blockIdx.x - cell * nchunk;
    const int cy = cell / ncx, cx = cell - cy * ncx;
    const int xa = bg_cell_start(cx, D.Wg, D.W), cw = bg_cell_start(cx + 1, D.Wg, D.W) - xa;
    const int ya = bg_cell_start(cy, D.Hg, D.H), ch = bg_cell_start(cy + 1, D.Hg, D.H) - ya;
    const int64_t npx = (int64_t)cw * ch, base = (int64_t)chunk * BG_CHUNK;
    if (base >= npx) return;   // the finish knows this cell's chunk count too
    const int one_x = D.Wg > 1, one_y = D.Hg > 1;
    const int nx = 1 + one_x, ny = 1 + one_y;

    float rgb[BG_PPL][3], go[BG_PPL][3], wxy[BG_PPL][4], fz[BG_PPL];
    int z0[BG_PPL];
    bool open[BG_PPL];
#pragma unroll
    for (int j = 0; j < BG_PPL; j++) {
        const int64_t i = base + j * BG_THREADS + tid;
        z0[j] = -2;   // no z node matches: the lane adds exact zeros
        open[j] = false;
        fz[j] = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) rgb[j][c] = go[j][c] = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; c++) wxy[j][c] = 0.0f;
        if (i >= npx) continue;
        const int ry = (int)(i / cw), px = xa + (int)(i - (int64_t)ry * cw), py = ya + ry;
        const size_t o = ((size_t)py * D.W + px) * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            rgb[j][c] = img[o + c];
            go[j][c] = gout[o + c];
        }
        const float fx = bg_frac(px, cx, D.Wg, D.W), fy = bg_frac(py, cy, D.Hg, D.H);
        int z1;
        bg_z(rgb[j][0], rgb[j][1], rgb[j][2], D.L, z0[j], z1, fz[j], open[j]);
        wxy[j][0] = (1.0f - fy) * (1.0f - fx);
        wxy[j][1] = (1.0f - fy) * fx;
        wxy[j][2] = fy * (1.0f - fx);
        wxy[j][3] = fy * fx;
    }
    // staged behind the pixel loads: the two latencies overlap
    if (STAGED && gimg != nullptr) bg_stage(s_g, 4 * BG_BWD_LMAX * 12, grid, D, cx, nx, cy, ny);
    if (gimg != nullptr) {
        // a real loop for the same reason as in the forward; the lane's pixel arrays rotate by one per trip and are
        // back in place after BG_PPL trips
#pragma unroll 1
        for (int j = 0; j < BG_PPL; j++) {
            const int64_t i = base + j * BG_THREADS + tid;
            if (i < npx) {
                const int ry = (int)(i / cw), px = xa + (int)(i - (int64_t)ry * cw), py = ya + ry;
                const size_t o = ((size_t)py * D.W + px) * 3;
                const float fx = bg_frac(px, cx, D.Wg, D.W), fy = bg_frac(py, cy, D.Hg, D.H);
                const int z1 = z0[0] + 1 < D.L ? z0[0] + 1 : D.L - 1;
                float A[12], dA[12];
                if (STAGED)
                    bg_interp<true>(s_g, 1, one_x * 12, one_y * nx * 12, nx * ny * 12, z0[0], z1, fx, fy, fz[0], A, dA);
                else
                    bg_interp<true>(grid + (size_t)cy * D.Wg + cx, D.L * D.Hg * D.Wg, one_x, one_y * D.Wg,
                                    D.Hg * D.Wg, z0[0], z1, fx, fy, fz[0], A, dA);
                float dz = 0.0f;
                if (open[0]) {
#pragma unroll
                    for (int r = 0; r < 3; r++)
                        dz += go[0][r] * (((dA[4 * r] * rgb[0][0] + dA[4 * r + 1] * rgb[0][1]) + dA[4 * r + 2] * rgb[0][2]) +
                                          dA[4 * r + 3]);
                    dz *= (float)(D.L - 1);
                }
                const float lum[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
                for (int c = 0; c < 3; c++)
                    gimg[o + c] = ((A[c] * go[0][0] + A[4 + c] * go[0][1]) + A[8 + c] * go[0][2]) + lum[c] * dz;
            }
            bg_rotate3(rgb);
            bg_rotate3(go);
            bg_rotate1(fz);
            bg_rotate1(z0);
            bg_rotate1(open);
        }
    }
    if (ws == nullptr) return;

    float* wsb = ws + (size_t)blockIdx.x * D.L * 48;
#pragma unroll 1
    for (int z = 0; z < D.L; z++) {
        float wz[BG_PPL];
        bool any = false;
#pragma unroll
        for (int j = 0; j < BG_PPL; j++) {
            // z1 = z0 + 1 on a guidance axis of two or more nodes; on one node both lerp ends are node 0
            wz[j] = (z == z0[j] ? 1.0f - fz[j] : 0.0f) + (z == z0[j] + 1 || (D.L == 1 && z0[j] == 0) ? fz[j] : 0.0f);
            any |= wz[j] != 0.0f;
        }
        if (__any(any)) {   // wave-uniform
            // pairs of accumulators: the products and sums below are two-wide packed fp32 instructions with the
            // roundings of the scalar ones (t * 1 is t)
            bg_f2 acc2[24];
#pragma unroll
            for (int i = 0; i < 24; i++) acc2[i] = bg_f2{0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < BG_PPL; j++) {
                const bg_f2 rg = {rgb[j][0], rgb[j][1]}, b1 = {rgb[j][2], 1.0f};
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const float w = wz[j] * wxy[j][c];
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const float t = w * go[j][r];
                        const bg_f2 t2 = {t, t};
                        acc2[c * 6 + 2 * r] += t2 * rg;
                        acc2[c * 6 + 2 * r + 1] += t2 * b1;
                    }
                }
            }
            float acc[48];   // [corner][4 r + j]
#pragma unroll
            for (int i = 0; i < 24; i++) {
                acc[2 * i] = acc2[i].x;
                acc[2 * i + 1] = acc2[i].y;
            }
            bg_halve<48>(acc, 1);
            bg_halve<24>(acc, 2);
            bg_halve<12>(acc, 4);
            bg_halve<6>(acc, 8);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                acc[i] += __shfl_xor(acc[i], 16);
                acc[i] += __shfl_xor(acc[i], 32);
            }
            if ((tid & 63) < 16) {
                const int off = (tid & 1) * 24 + ((tid >> 1) & 1) * 12 + ((tid >> 2) & 1) * 6 + ((tid >> 3) & 1) * 3;
#pragma unroll
                for (int i = 0; i < 3; i++) s_red[tid >> 6][off + i] = acc[i];
            }
        } else if ((tid & 63) < 48) {
            s_red[tid >> 6][tid & 63] = 0.0f;
        }
        __syncthreads();
        if (tid < 48) wsb[z * 48 + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
        __syncthreads();
    }
}

// grad_grid[k, z, y, x] = the partials of corner (y - cy, x - cx) of the cells cy in {y - 1, y}, cx in {x - 1, x},
// cells and chunks in index order.  A chunk index past a cell's count reads a valid address and adds an exact zero,
// so the loads of one cell are independent of each other.
__global__ __launch_bounds__(BG_THREADS) void k_bilagrid_grad_finish(const float* __restrict__ ws, BgDims D, int ncx,
                                                                     int ncy, int nchunk, float* __restrict__ gg) {
    // the channel runs fastest over the lanes: a partial's 12 channels are consecutive floats
    const int e = blockIdx.x * BG_THREADS + threadIdx.x;
    if (e >= 12 * D.L * D.Hg * D.Wg) return;
    const int k = e % 12, node = e / 12;
    const int x = node % D.Wg, y = (node / D.Wg) % D.Hg, z = node / (D.Wg * D.Hg);
    float sum = 0.0f;
    for (int dy = 1; dy >= 0; dy--)
        for (int dx = 1; dx >= 0; dx--) {
            const int cy = y - dy, cx = x - dx;
            if (cy < 0 || cy >= ncy || cx < 0 || cx >= ncx || (dy && D.Hg < 2) || (dx && D.Wg < 2)) continue;
            const int64_t npx = (int64_t)(bg_cell_start(cx + 1, D.Wg, D.W) - bg_cell_start(cx, D.Wg, D.W)) *
                                (bg_cell_start(cy + 1, D.Hg, D.H) - bg_cell_start(cy, D.Hg, D.H));
            const int count = (int)((npx + BG_CHUNK - 1) / BG_CHUNK);
            if (count == 0) continue;
            const float* p = ws + ((size_t)(cy * ncx + cx) * nchunk * D.L + z) * 48 + (dy * 2 + dx) * 12 + k;
#pragma unroll 4
            for (int c = 0; c < nchunk; c++) {
                const float v = p[(size_t)(c < count ? c : 0) * D.L * 48];
                sum += c < count ? v : 0.0f;
            }
        }
    gg[(((size_t)k * D.L + z) * D.Hg + y) * D.Wg + x] = sum;
}

// ---- total variation ----------------------------------------------------------------------------------------------
// grids: n planes of [L, Hg, Wg].  value = sum over the axes of two or more nodes of mean (forward difference)^2;
// icx / icy / icz: 1 / (number of adjacent pairs on the axis), 0 for an axis of one node.
__global__ __launch_bounds__(BG_THREADS) void k_bilagrid_tv(const float* __restrict__ g, int64_t total, int L, int Hg,
                                                            int Wg, double icx, double icy, double icz,
                                                            double* __restrict__ partial, float* __restrict__ grad) {
    __shared__ double s_red[BG_THREADS / GS_WAVE];
    const int64_t e0 = (int64_t)blockIdx.x * (BG_THREADS * BG_TV_PER);
    const unsigned S = (unsigned)L * Hg * Wg;   // one plane; < 2^31 / 12
    const unsigned r0 = (unsigned)(e0 % S);     // wave-uniform: the 64-bit division is scalar
    const int sy = Wg, sz = Wg * Hg;
    double val = 0.0;
#pragma unroll 4
    for (int t = 0; t < BG_TV_PER; t++) {
        const unsigned off = (unsigned)t * BG_THREADS + threadIdx.x;
        const int64_t e = e0 + off;
        if (e >= total) break;
        const unsigned r = (r0 + off) % S;
        const int x = (int)(r % (unsigned)Wg), y = (int)((r / (unsigned)Wg) % (unsigned)Hg), z = (int)(r / (unsigned)sz);
        const float c = g[e];
        // differences to the next and from the previous node; exact zeros at the ends
        const double nx = x + 1 < Wg ? (double)(g[e + 1] - c) : 0.0, px = x > 0 ? (double)(c - g[e - 1]) : 0.0;
        const double ny = y + 1 < Hg ? (double)(g[e + sy] - c) : 0.0, py = y > 0 ? (double)(c - g[e - sy]) : 0.0;
        const double nz = z + 1 < L ? (double)(g[e + sz] - c) : 0.0, pz = z > 0 ? (double)(c - g[e - sz]) : 0.0;
        val += (nx * nx) * icx + (ny * ny) * icy + (nz * nz) * icz;
        if (grad != nullptr) grad[e] = (float)(2.0 * (((px - nx) * icx + (py - ny) * icy) + (pz - nz) * icz));
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) val += __shfl_xor(val, d);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = val;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

__global__ __launch_bounds__(BG_THREADS) void k_bilagrid_tv_finish(const double* __restrict__ partial, int64_t n,
                                                                   float* __restrict__ out) {
    __shared__ double s[BG_THREADS];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += BG_THREADS) a += partial[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int d = BG_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)s[0];
}

// cells per axis and the chunks of the largest cell
static void bg_partition(int H, int W, int Hg, int Wg, int& ncx, int& ncy, int& nchunk) {
    ncx = Wg > 1 ? Wg - 1 : 1;
    ncy = Hg > 1 ? Hg - 1 : 1;
    int mw = 0, mh = 0;
    for (int c = 0; c < ncx; c++) {
        const int w = bg_cell_start(c + 1, Wg, W) - bg_cell_start(c, Wg, W);
        mw = w > mw ? w : mw;
    }
    for (int c = 0; c < ncy; c++) {
        const int h = bg_cell_start(c + 1, Hg, H) - bg_cell_start(c, Hg, H);
        mh = h > mh ? h : mh;
    }
    nchunk = (int)(((int64_t)mw * mh + BG_CHUNK - 1) / BG_CHUNK);
    if (nchunk < 1) nchunk = 1;
}

}  // namespace gs

using namespace gs;

#define BG_REQUIRE_DIMS(what)                                                                                        \
    GS_REQUIRE(H >= 1 && W >= 1 && L >= 1 && Hg >= 1 && Wg >= 1, what ": H, W, L, Hg, Wg must be >= 1");            \
    GS_REQUIRE(W < (1 << 23) && H < (1 << 23) && (int64_t)W * Wg < (1 << 30) && (int64_t)H * Hg < (1 << 30),         \
               what ": the image is too large for 32-bit cell arithmetic");                                          \
    GS_REQUIRE((int64_t)12 * L * Hg * Wg < ((int64_t)1 << 31), what ": the grid is too large")

extern "C" {

size_t gs_bilagrid_workspace_bytes(int H, int W, int L, int Hg, int Wg) {
    if (H < 1 || W < 1 || L < 1 || Hg < 1 || Wg < 1) return 0;
    int ncx, ncy, nchunk;
    bg_partition(H, W, Hg, Wg, ncx, ncy, nchunk);
    return (size_t)ncx * ncy * nchunk * L * 48 * sizeof(float);
}

int gs_bilagrid_slice(const void* grid, const void* image, int H, int W, int L, int Hg, int Wg, void* out,
                      void* stream) {
    BG_REQUIRE_DIMS("bilagrid_slice");
    GS_REQUIRE(grid != nullptr && image != nullptr && out != nullptr, "bilagrid_slice: grid, image and out are required");
    const BgDims D = {H, W, L, Hg, Wg};
    const dim3 tiles(div_up(W, BG_TX), div_up(H, BG_TY));
    GS_REQUIRE(tiles.y < 65536u, "bilagrid_slice: the image is too tall");
    const int64_t box = (int64_t)bg_nodes_bound(BG_TX, Wg, W) * bg_nodes_bound(BG_TY, Hg, H) * L * 12;
    hipStream_t s = (hipStream_t)stream;
    if (box <= BG_FWD_LDS)
        k_bilagrid_slice<true><<<tiles, BG_THREADS, 0, s>>>((const float*)grid, (const float*)image, D, (float*)out);
    else
        k_bilagrid_slice<false><<<tiles, BG_THREADS, 0, s>>>((const float*)grid, (const float*)image, D, (float*)out);
    return check_launch("bilagrid_slice");
}

int gs_bilagrid_slice_backward(const void* grid, const void* image, const void* grad_out, int H, int W, int L, int Hg,
                               int Wg, void* workspace, void* grad_image, void* grad_grid, void* stream) {
    BG_REQUIRE_DIMS("bilagrid_slice_backward");
    GS_REQUIRE(grid != nullptr && image != nullptr && grad_out != nullptr,
               "bilagrid_slice_backward: grid, image and grad_out are required");
    GS_REQUIRE(grad_grid == nullptr || workspace != nullptr,
               "bilagrid_slice_backward: grad_grid needs the workspace of gs_bilagrid_workspace_bytes");
    if (grad_image == nullptr && grad_grid == nullptr) return GS_OK;
    const BgDims D = {H, W, L, Hg, Wg};
    int ncx, ncy, nchunk;
    bg_partition(H, W, Hg, Wg, ncx, ncy, nchunk);
    const int64_t blocks = (int64_t)ncx * ncy * nchunk;
    GS_REQUIRE(blocks < ((int64_t)1 << 31), "bilagrid_slice_backward: too many cell chunks");
    hipStream_t s = (hipStream_t)stream;
    float* ws = grad_grid != nullptr ? (float*)workspace : nullptr;
    if (L <= BG_BWD_LMAX)
        k_bilagrid_slice_bwd<true><<<(unsigned)blocks, BG_THREADS, 0, s>>>(
            (const float*)grid, (const float*)image, (const float*)grad_out, D, ncx, nchunk, ws, (float*)grad_image);
    else
        k_bilagrid_slice_bwd<false><<<(unsigned)blocks, BG_THREADS, 0, s>>>(
            (const float*)grid, (const float*)image, (const float*)grad_out, D, ncx, nchunk, ws, (float*)grad_image);
    if (grad_grid != nullptr)
        k_bilagrid_grad_finish<<<div_up(12 * L * Hg * Wg, BG_THREADS), BG_THREADS, 0, s>>>(ws, D, ncx, ncy, nchunk,
                                                                                          (float*)grad_grid);
    return check_launch("bilagrid_slice_backward");
}

size_t gs_bilagrid_tv_workspace_bytes(int64_t n_grids, int L, int Hg, int Wg) {
    if (n_grids < 1 || L < 1 || Hg < 1 || Wg < 1) return 0;
    const int64_t total = n_grids * 12 * L * Hg * Wg;
    return (size_t)((total + BG_THREADS * BG_TV_PER - 1) / (BG_THREADS * BG_TV_PER)) * sizeof(double);
}

int gs_bilagrid_tv(const void* grids, int64_t n_grids, int L, int Hg, int Wg, void* workspace, void* tv_out,
                   void* grad_grids, void* stream) {
    GS_REQUIRE(n_grids >= 1 && L >= 1 && Hg >= 1 && Wg >= 1, "bilagrid_tv: n_grids, L, Hg, Wg must be >= 1");
    GS_REQUIRE(grids != nullptr && workspace != nullptr && tv_out != nullptr,
               "bilagrid_tv: grids, workspace and tv_out are required");
    const int64_t planes = n_grids * 12, total = planes * L * Hg * Wg;
    const int64_t blocks = (total + BG_THREADS * BG_TV_PER - 1) / (BG_THREADS * BG_TV_PER);
    GS_REQUIRE((int64_t)12 * L * Hg * Wg < ((int64_t)1 << 31), "bilagrid_tv: the grid is too large");
    GS_REQUIRE(blocks < ((int64_t)1 << 31), "bilagrid_tv: too many grids");
    const double icx = Wg > 1 ? 1.0 / ((double)planes * L * Hg * (Wg - 1)) : 0.0;
    const double icy = Hg > 1 ? 1.0 / ((double)planes * L * (Hg - 1) * Wg) : 0.0;
    const double icz = L > 1 ? 1.0 / ((double)planes * (L - 1) * Hg * Wg) : 0.0;
    hipStream_t s = (hipStream_t)stream;
    k_bilagrid_tv<<<(unsigned)blocks, BG_THREADS, 0, s>>>((const float*)grids, total, L, Hg, Wg, icx, icy, icz,
                                                          (double*)workspace, (float*)grad_grids);
    k_bilagrid_tv_finish<<<1, BG_THREADS, 0, s>>>((const double*)workspace, blocks, (float*)tv_out);
    return check_launch("bilagrid_tv");
}

}  // extern "C"
