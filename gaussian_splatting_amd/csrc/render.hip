// render.hip -- tile renderer for gfx950: forward compositing, backward, depth.
//
// Replaces render_tiles_kernel (render.cu:8-189), render_tiles_backward_kernel
// (render_backward.cu:12-285) and render_depth_kernel (depth.cu:7-115).
//
// Mapping.  One 256-thread workgroup (4 waves) per 16x16 tile; wave w owns the 8x8 pixel
// quadrant (w&1, w>>1), lane l the pixel (l&7, l>>3) inside it, so that a wave covers a compact
// patch: a splat that misses the patch is skipped by the whole wave with one ballot.  Workgroups
// are laid out so that each XCD renders a contiguous band of tiles (block b runs on XCD b%8):
// neighbouring tiles share Gaussians and hit the same 4 MiB L2.
//
// Data flow.  Per chunk of splats (256 in the fused forward, 64 in its backward) the workgroup gathers the
// 48-byte packed record (gs_pack_splats / gs_preprocess_forward: u v r2 opacity | a b c det | 1/det colour --
// three 16-byte loads; or forms it from the reference's separate arrays, stage_chunk) and, for per-pixel SH,
// the colour coefficients of the depth-sorted Gaussians into LDS; every thread then tests the record it
// staged against the tile's four 8x8 patches (build_touch_masks) and a wave walks only the splats whose
// cutoff ellipse reaches its patch, with wave-uniform (broadcast) LDS reads.  Barriers are uniform
// (Q2 of SURVEY.md is not replicated).  Forward leaves the chunk loop as soon as every pixel of the tile is
// saturated (result-preserving: a saturated pixel ignores all later splats, render.cu:106).
//
// Forward: two bodies.
//   render_tile_fwd_fused<CK>, fp32 with one colour coefficient -- the fused renderer's, in k_render_fwd<float, 1>,
//   k_render_fwd_ck (CK: leaves the depth-segment state for the backward) and k_render_fwd_flagged<CK> (repair pass);
//   also what gs_render_tiles / gs_render_tiles_packed run for float32 with n_sh == 1.  The record of the next visit
//   is requested while the current one is composited (lds_record_fetch, b + b staged in the record).  It alone
//   carries the prefix mode, the depth cut, tile_flags / flag_counter, the speculative list capacity, the tile costs
//   and the touch masks handed to the backward.
//   render_tile_fwd_general<T, N_SH> in k_render_fwd_general, every other pair (float at 4 / 9 / 16 coefficients,
//   double at 1 / 4 / 9 / 16: gradcheck and the parity tests): whole lists, the plain walk -- one record read per
//   visit -- and the colour from the staged coefficients at the pixel's view direction (sh_basis, splat_colour).
//
// Prefix mode (binning.hip "prefix sort"): a long tile list may have only its 1024 nearest entries
// ordered; the fused forward reads no further, raises tile_flags[t] if a pixel is still unsaturated there,
// and k_render_fwd_flagged renders such tiles again after their full sort -- results are exact.
//
// Backward: three kernels, each with its walk written out.  All start at the tile's largest num_splats_per_pixel
// instead of the end of the list and skip the reduction for waves none of whose lanes the splat reaches.
//   k_render_bwd<float, 1>, fp32 with one colour coefficient -- the fused renderer's, and what gs_render_tiles_backward /
//   _packed run for float32 with n_sh == 1: sums nine per-splat values over the wave with a transposing DPP /
//   permlane-swap reduction into a wave-private LDS slot (plain store, no LDS atomics); the flush adds the four waves'
//   slots (flush_sum_slots' text, written out here; the routine itself in the other fp32 backwards) and issues the
//   global atomics nine lanes per 36-byte row (of the [V, 9] slab, or of the separate gradient arrays).  It alone
//   carries the fused frame's depth
//   segments, depth-cut overflow lists, handed-over touch masks and the longest-first tile order (durations the forward
//   measured; k_bwd_prologue: tile_order_body).
//   k_render_bwd_sh<N_SH>, fp32 with per-pixel SH (4 / 9 / 16 coefficients): the same slots for the six geometric sums,
//   whole lists, separate gradient arrays; the colour is evaluated at the pixel's view direction and the
//   colour-coefficient gradients are a matrix-core contraction over the wave's 64 pixels per batch of 16 contributing
//   splats.
//   k_render_bwd_ref<N_SH>, fp64 (gradcheck and the fp64 parity tests): one shared LDS row of 3 N_SH + 6 sums per
//   staged splat, shuffle wave sums + one LDS atomic per value per visit, one global atomic per value per
//   (splat, tile) -- the reference issues eight (one per warp), unconditionally.
//
// Maps (no reference counterpart): depth / alpha (k_render_zalpha_fwd / _bwd) and per-Gaussian feature vectors
// (k_render_features_fwd / _bwd<CP>) composited with the weights of the entries the colour forward walked.  One
// forward walk and one backward walk with its flush, render_map_fwd / render_map_bwd, templated on a channel policy
// that holds what a family has of its own: where the channel values come from and where their sums and gradients go.
// The depth distortion (k_render_distortion_fwd / _bwd) is the depth map's walk with two more sums: its forward is a
// policy of render_map_fwd, its backward a policy of render_map_bwd (DistortionBwd, whose c_k needs w_k: the c() hook
// is handed what forms it).  The median depth (k_render_median_fwd) is the depth map's forward with a (z, index) pair
// that every contributor in front of which T is still above one half overwrites: the add() hook is handed T; its
// backward (k_median_depth_bwd) is a scatter without a walk.
//
// Numerics.  The fp32 forward is bit-identical to the CPU restatement: same operation order and
// operand precisions as render.cu (including its double-literal promotions), the IEEE quotient (formed
// from the stored reciprocal, div_by_reciprocal), det_expf in place of __expf.  Backward forms alpha and
// the skip decisions bit-identically (render_backward.cu:141-170) and evaluates the gradient formulas in T.
#include "pg_math.h"
#include "tile_sort.h"
#include <atomic>

namespace gs {

// Instrumented build only (make stats: -DGS_STATS -> libgsplat_hip_stats.so, scripts/render_stats.py):
// per-wave event counts of the render kernels, summed into g_render_stats.  Expands to nothing in
// the product library.
#ifdef GS_STATS
__device__ unsigned long long g_render_stats[32];
// wave timeline (scripts/render_timeline.py, -DGS_STATS -DGS_TIMELINE): one record {begin, end, hw id |
// xcc id, visits, chunks} per wave at slot (kernel, block, wave), times from the 100 MHz constant clock.
// The timeline build does not add to the shared counters (their atomics serialise the waves' exits).
constexpr int GS_TIMELINE_CAP = 1 << 16;   // waves per kernel
constexpr int GS_TIMELINE_W = 10;
__device__ unsigned long long g_timeline[2 * GS_TIMELINE_CAP * GS_TIMELINE_W];
#define GS_STAT_DECL                                                                               \
    unsigned long long st_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                  \
    const unsigned long long st_t0_ = wall_clock64();                                             \
    const unsigned long long st_c0_ = __builtin_readcyclecounter();                                \
    unsigned long long st_ph_ = st_c0_;                                                            \
    (void)st_t0_;                                                                                  \
    (void)st_c0_;                                                                                  \
    (void)st_ph_
#define GS_STAT_FLAG(name) bool name = false
#define GS_STAT_SET(name) name = true
#ifdef GS_TIMELINE
#define GS_STAT(i, v)                                                                              \
    if ((i) == 1 || (i) == 2) st_[i] += (unsigned long long)(v)
// cycles since the previous mark go to phase k (k = 0..4)
#define GS_PHASE(k)                                                                                \
    {                                                                                              \
        const unsigned long long c_ = __builtin_readcyclecounter();                                \
        st_[10 + (k)] += c_ - st_ph_;                                                              \
        st_ph_ = c_;                                                                               \
    }
#define GS_STAT_FLUSH(base)                                                                        \
    if ((threadIdx.x & 63) == 0) {                                                                 \
        const unsigned r_ = blockIdx.x * 4 + (threadIdx.x >> 6);                                   \
        if (r_ < (unsigned)GS_TIMELINE_CAP) {                                                      \
            unsigned long long* t_ = g_timeline + ((size_t)((base) ? GS_TIMELINE_CAP : 0) + r_) * GS_TIMELINE_W; \
            for (int q_ = 0; q_ < 5; q_++) t_[5 + q_] = st_[10 + q_];                              \
            t_[0] = st_t0_;                                                                        \
            t_[1] = wall_clock64();                                                                \
            t_[2] = ((unsigned long long)__builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11)) << 32) | \
                    (unsigned)__builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));              \
            t_[3] = st_[2];                                                                        \
            t_[4] = (st_[1] << 48) | ((__builtin_readcyclecounter() - st_c0_) & 0xffffffffffffull);   \
        }                                                                                          \
    }
#else
#define GS_PHASE(k)
#define GS_STAT(i, v) st_[i] += (unsigned long long)(v)
// what two independent 8x4 half-waves in lockstep would walk: per chunk, the visits in which the upper
// / the lower half of the patch has a lane inside the cutoff circle; the lockstep walk takes the larger of the two
#define GS_HALF_DECL unsigned st_ha_ = 0, st_hb_ = 0
#define GS_HALF_VISIT(bal)                                                                         \
    {                                                                                              \
        const unsigned long long b_ = (bal);                                                       \
        st_ha_ += (b_ & 0xffffffffull) != 0;                                                       \
        st_hb_ += (b_ >> 32) != 0;                                                                 \
    }
#define GS_HALF_CHUNK(i)                                                                           \
    {                                                                                              \
        st_[i] += st_ha_ > st_hb_ ? st_ha_ : st_hb_;                                               \
        st_[(i) + 1] += st_ha_;                                                                    \
        st_[(i) + 2] += st_hb_;                                                                    \
        st_ha_ = st_hb_ = 0;                                                                       \
    }
#define GS_STAT_FLUSH(base)                                                                        \
    if ((threadIdx.x & 63) == 0) {                                                                 \
        for (int q_ = 0; q_ < 16; q_++)                                                            \
            if (st_[q_]) atomicAdd(&g_render_stats[(base) + q_], st_[q_]);                         \
    }
#endif
#else
#define GS_STAT_DECL
#define GS_STAT(i, v)
#define GS_STAT_FLAG(name)
#define GS_STAT_SET(name)
#define GS_STAT_FLUSH(base)
#define GS_PHASE(k)
#endif
#ifndef GS_HALF_DECL
#define GS_HALF_DECL
#define GS_HALF_VISIT(bal)
#define GS_HALF_CHUNK(i)
#endif

#ifndef GS_BWD_CHUNK
// splats staged per step by the fused renderer's backward.  64: 12.5 KB of LDS and 71 VGPRs = 7 waves per
// SIMD (128: 25 KB and 78 VGPRs = 6; 0.514 -> 0.505 ms at D, 0.155 -> 0.149 at B; with amdgpu_waves_per_eu(8)
// the compiler reaches 64 VGPRs without spilling but the kernel is no faster)
#define GS_BWD_CHUNK 64
#endif
constexpr int RB = 256;      // workgroup size = pixels per tile
// (experiment builds: bytes of unused dynamic LDS per workgroup of the fused frame's render kernels -- caps the
// workgroups a CU holds, i.e. trades waves in flight for shorter-lived ones; profiles/r04/kbench_lds_pad.txt)
#ifndef GS_FWD_LDS_PAD
#define GS_FWD_LDS_PAD 0
#endif
#ifndef GS_BWD_LDS_PAD
#define GS_BWD_LDS_PAD 0
#endif

// splats staged in LDS per step (at most one per thread); smaller for the wide test-only
// instantiations so that every kernel stays below 64 KiB of static LDS
#ifndef GS_FWD_CHUNK
#define GS_FWD_CHUNK 256   // the fp32 one-coefficient forward (the fused renderer's); 128: +3 %, 64: +9 % at D
#endif
template <typename T, int N_SH> struct Chunk {
    static constexpr int value = (sizeof(T) * N_SH <= 4) ? GS_FWD_CHUNK : (sizeof(T) * N_SH <= 8) ? 256 : (sizeof(T) * N_SH <= 36) ? 128 : 64;
};

template <typename T> struct alignas(16) Vec4 { T x, y, z, w; };

template <int N_SH> struct ColW { static constexpr int value = (3 * N_SH + 3) & ~3; };

// reference chunk sizes, needed only for bug-compatibility with render_backward.cu:185 (Q1)
template <typename T> __host__ __device__ constexpr int ref_chunk(int n_sh);
template <> __host__ __device__ constexpr int ref_chunk<float>(int n_sh) {
    return n_sh == 1 ? 960 : n_sh == 4 ? 576 : n_sh == 9 ? 320 : 160;
}
template <> __host__ __device__ constexpr int ref_chunk<double>(int n_sh) {
    return n_sh == 1 ? 320 : n_sh == 4 ? 160 : n_sh == 9 ? 128 : 64;
}

// XCD-aware tile order: block b -> tile index inside [0, nt) (or >= nt: nothing to do).  The hardware
// hands block b to XCD b % 8, a fixed eighth of the grid each.  Default: one contiguous eighth of the
// frame per XCD (its L2 holds the records neighbouring tiles share).  Dealing runs of 8 / 16 / 32 / 82 consecutive
// tiles to the XCDs in turn instead was measured (scripts/experiments/render_macro_experiments.patch, its XCD_SEG option;
// profiles/r02/kbench_xcd_segments.log): kernel times within 1.5 %, not kept.
__host__ __device__ inline int render_grid(int nt) {
    return ((nt + 7) / 8) * 8;
}
__device__ inline int tile_of_block(int b, int nt) {
    const int per = (nt + 7) >> 3;
    return (b & 7) * per + (b >> 3);
}

struct PixelMap {
    int u, v;
};
__device__ inline PixelMap pixel_of_thread(int tile_x, int tile_y, int tid) {
    const int w = tid >> 6, l = tid & 63;
    PixelMap p;
    p.u = tile_x * 16 + ((w & 1) << 3) + (l & 7);
    p.v = tile_y * 16 + ((w >> 1) << 3) + (l >> 3);
    return p;
}

// gather one chunk of splats into LDS: the 12-scalar packed record (three 16-byte loads) and, for
// N_SH > 1, the [3, N_SH] colour coefficients.  s_idx (optional) keeps the Gaussian indices.
// src_opacity != nullptr: the splats come as the reference's separate arrays (render_tiles_cuda's
// uvs / opacity / conic / rgb: `packed` is then uvs[V,2]) and the record is formed here, with the
// function gs_pack_splats uses -- the same values, no packing pass and no [V,12] buffer for the caller.
// TWO_B: the cross term's factor b + b (render.cu:129, render_backward.cu:155) is the same for every pixel -- one add per
// staged record where it was one per visit.  1 (the backward, which never reads det): in word 7 of the staged record;
// 2 (the pipelined forward, which needs det): in word 5, INSTEAD of b -- its only other reader, the touch-mask test of
// the same thread, halves it again (exact).
template <typename T, int N_SH, int TWO_B = 0>
__device__ inline void stage_chunk(const T* __restrict__ packed, const T* __restrict__ rgb,
                                   const int* __restrict__ sorted, int first, int count, int tid,
                                   T* s_geom, T* s_col, int* s_idx, const T* __restrict__ src_opacity = nullptr,
                                   const T* __restrict__ src_conic = nullptr) {
    constexpr int CW = ColW<N_SH>::value;
    if (tid < count) {
        const int g = sorted[first + tid];
        if (src_opacity != nullptr) {
            const T c3[3] = {src_conic[(size_t)g * 3 + 0], src_conic[(size_t)g * 3 + 1], src_conic[(size_t)g * 3 + 2]};
            T col[3] = {0, 0, 0};
            if constexpr (N_SH == 1) {
                col[0] = rgb[(size_t)g * 3 + 0]; col[1] = rgb[(size_t)g * 3 + 1]; col[2] = rgb[(size_t)g * 3 + 2];
            }
            T p[GS_PACKED_WIDTH];
            pack_record<T>(packed[(size_t)g * 2 + 0], packed[(size_t)g * 2 + 1], c3, src_opacity[g], col, p);
#pragma unroll
            for (int k = 0; k < GS_PACKED_WIDTH; k++) s_geom[tid * GS_PACKED_WIDTH + k] = p[k];
        } else {
            const Vec4<T>* src = reinterpret_cast<const Vec4<T>*>(packed + (size_t)g * GS_PACKED_WIDTH);
            Vec4<T>* dst = reinterpret_cast<Vec4<T>*>(s_geom + tid * GS_PACKED_WIDTH);
            dst[0] = src[0];
            dst[1] = src[1];
            dst[2] = src[2];
        }
        if constexpr (TWO_B != 0) {
            const T b = s_geom[tid * GS_PACKED_WIDTH + 5];
            s_geom[tid * GS_PACKED_WIDTH + (TWO_B == 1 ? 7 : 5)] = b + b;
        }
        if (s_idx) s_idx[tid] = g;
    }
    if constexpr (N_SH > 1) {
        // the [3, N_SH] coefficient rows, by the whole workgroup: consecutive threads read consecutive words of
        // a row (one thread per row with 3 N_SH dependent-latency loads was 0.2 ms of the 0.4 ms skeleton of the
        // N_SH = 16 backward at workload B)
        constexpr int C = 3 * N_SH;
        for (int k = tid; k < count * C; k += RB) {
            const int r = k / C, c = k - r * C;
            s_col[r * CW + c] = rgb[(size_t)sorted[first + r] * C + c];
        }
    }
}

template <typename T> __device__ constexpr bool fast_mode() { return sizeof(T) == 4; }

// wave ballot straight from the comparison's lane mask (HIP's __ballot first materialises the
// predicate as an integer: v_cndmask + v_cmp per call)
__device__ __forceinline__ unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// exp(-0.5 * mh) of the render loops (render.cu:134, render_backward.cu:160), fp32: det_expf without
// its range selects.  -0.5 * mh is exact, so t below is the same single rounding as det_expf's; for
// t > -125 the remaining operations are det_expf's own, bit for bit.  Below that both values are
// < 2^-100, and in fp32 the callers only use such a value through `opacity * value < 1/255`
// (render.cu:145, render_backward.cu:170), which it fails either way.  mh > 0 and not NaN here.
__device__ __forceinline__ float exp_neg_half(float mh) {
    const float t = mh * (-0.5f * 1.44269504088896341f);
    const float n = __builtin_rintf(t);
    const float f = t - n;
    float p = 1.54035303933816e-4f;
    p = __builtin_fmaf(p, f, 1.33335581464284e-3f);
    p = __builtin_fmaf(p, f, 9.61812910762848e-3f);
    p = __builtin_fmaf(p, f, 5.55041086648216e-2f);
    p = __builtin_fmaf(p, f, 2.40226506959101e-1f);
    p = __builtin_fmaf(p, f, 6.93147180559945e-1f);
    p = __builtin_fmaf(p, f, 1.0f);
    return __builtin_ldexpf(p, (int)n);
}
__device__ __forceinline__ double exp_neg_half(double mh) { return exp(-0.5 * mh); }

// q / det, correctly rounded, from the correctly rounded reciprocal r = RN(1 / det) of the packed
// record ((float)(1.0 / (double)det) equals 1.0f / det for every float): y = RN(q r),
// e = q - det y (exact in one fma), RN(y + e r) is the IEEE quotient (Markstein) for every normal
// q, det with a normal quotient -- 3 instructions instead of the 10 of the division expansion.
// Checked against `/` on 3.2e9 random and edge-mantissa pairs.  Where the quotient
// overflows or det is 0 the result is NaN instead of +-inf; `mh > 0` is then false where the
// reference finds exp(-inf) = 0: alpha = 0 either way.
__device__ __forceinline__ float div_by_reciprocal(float q, float det, float r) {
    const float y = q * r;
    const float e = __builtin_fmaf(-det, y, q);
    return __builtin_fmaf(e, r, y);
}
__device__ __forceinline__ double div_by_reciprocal(double q, double det, double) { return q / det; }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ double fast_rcp(double x) { return 1.0 / x; }
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ double fast_sqrt(double x) { return sqrt(x); }
// background weight of the backward's first contributor, render_backward.cu:175:
//     const T background_weight = 1.0 - (alpha * weight + 1.0 - weight);
// fp32: x = alpha * weight is a float product; the double literals promote the rest -- (x + 1.0) - weight, then 1.0 - that
// -- and the result is narrowed to float.  With alpha in [1/255, 0.9999] (the branch it sits in) and weight = the
// forward's final weight 1 - acc in [1e-4, 1], x and weight are multiples of 2^-45 below 2, so every one of the three
// double operations is EXACT (46 bits of 53) and the value narrowed is weight - x itself: RN_float(weight - x), which is
// what one IEEE float subtraction returns.  One v_sub_f32 for 2 conversions + 3 fp64 adds + the conversion back (fp64-rate
// instructions, ~4 cycles each, executed in every visit in which some pixel of the wave meets its first contributor);
// bit-identical (4e8 random and edge-mantissa pairs on the host: tests/test_host_logic.py holds a sample).
template <typename T> __device__ __forceinline__ T background_weight(T alpha, T weight);
template <> __device__ __forceinline__ float background_weight<float>(float alpha, float weight) {
    const float x = alpha * weight;
    return weight - x;
}
template <> __device__ __forceinline__ double background_weight<double>(double alpha, double weight) {
    return 1.0 - (alpha * weight + 1.0 - weight);
}

// a register the compiler must treat as defined without an instruction that defines it (its content is whatever the
// lane held): for values only SOME lanes compute and the others are masked out of afterwards
__device__ __forceinline__ float unset() {
    float x;
    asm volatile("" : "=v"(x));
    return x;
}
// a * b with 0 * x = 0 for EVERY x (v_mul_legacy_f32: NaN and infinity included): the masked-out factor of a lane may be
// anything.  Equal to a * b whenever both are finite
__device__ __forceinline__ float mul_zero_wins(float a, float b) {
    float r;
    asm("v_mul_legacy_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <typename T> __device__ inline T tmin(T a, T b) { return b < a ? b : a; }
template <typename T> __device__ inline T tmax(T a, T b) { return b > a ? b : a; }

// moves a wave-uniform 64-bit value into scalar registers
__device__ inline unsigned long long wave_uniform(unsigned long long m) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)m);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(m >> 32));
    return ((unsigned long long)hi << 32) | (unsigned long long)lo;
}

// Per-chunk wave-level touch masks.  Thread t tests the cutoff circle (centre u,v, radius^2 r2) of
// staged splat t against the four 8x8 pixel patches of the tile; ballots turn that into one 64-bit
// mask per (patch, 64 splats).  A wave then visits only the splats whose mask bit is set.  Exactly
// result-preserving: the patch distance (dx, dy) is the per-pixel (du, dv) of the nearest pixel or
// 0, float multiply/add are monotone, so dx*dx + dy*dy > r2 implies du*du + dv*dv > r2 for every
// pixel of the patch, i.e. every lane would have taken the "alpha < 1/255" path.  NaNs compare
// false and keep the splat.
template <typename T, int CHUNK, bool B_DOUBLED = false>
__device__ inline void build_touch_masks(const T* s_geom, int cnt, int tid, int tile_x, int tile_y,
                                         unsigned long long (*s_mask)[CHUNK / 64 > 0 ? CHUNK / 64 : 1]) {
    if (tid < CHUNK) {   // CHUNK <= 256 == workgroup size
        unsigned touch = 0;
        if (tid < cnt) {
            const T* rec = s_geom + tid * GS_PACKED_WIDTH;
            const T u = rec[0], v = rec[1], r2 = rec[2];
            // Exact test of the cutoff ellipse {d : d' S^-1 d <= tau_m} against each patch rectangle:
            // the minimum of q(d) = (c dx^2 - 2 b dx dy + a dy^2) / det over the rectangle of pixel
            // offsets is 0 if the centre lies inside, else it is attained on an edge, where q is a
            // 1-D parabola.  tau_m = r2 / lmax >= 1.05 tau (r2 carries the margin of cutoff_r2), and
            // the continuous minimum bounds every pixel's q from below, so q_min > tau_m means no
            // pixel of the patch can reach alpha >= 1/255.  Cheaper bounds first (circle).
            // (b/a, b/c, 1/lmax from the hardware reciprocal, 1 ulp: where the clamped minimiser lands
            // 1e-7 off, q exceeds the true edge minimum by a second-order 1e-14 -- the 1.001 on tau_m and
            // the 5 % margin inside r2 cover that a million times over.  17 IEEE divisions per splat and
            // chunk were 14 % of the forward kernel's wave time.)
            bool use_q = false;
            T a = 0, b = 0, c = 0, rdet = 0, tau_m = 0, b_over_a = 0, b_over_c = 0;
            if (fast_mode<T>() && r2 > T(0) && r2 < T(1e30)) {
                a = rec[4]; b = B_DOUBLED ? T(0.5) * rec[5] : rec[5]; c = rec[6]; rdet = rec[8];
                const T half = T(0.5) * (a + c);
                const T lmax = half + fast_sqrt(T(0.25) * (a - c) * (a - c) + b * b);
                tau_m = (r2 * fast_rcp(lmax)) * T(1.001);
                use_q = a > T(0) && c > T(0) && rdet > T(0);
                b_over_a = b * fast_rcp(a);
                b_over_c = b * fast_rcp(c);
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const T x0 = T(tile_x * 16 + ((p & 1) << 3)), y0 = T(tile_y * 16 + ((p >> 1) << 3));
                const T x1 = x0 + T(7), y1 = y0 + T(7);
                T dx = T(0), dy = T(0);
                if (u < x0) dx = x0 - u;
                if (u > x1) dx = x1 - u;
                if (v < y0) dy = y0 - v;
                if (v > y1) dy = y1 - v;
                bool hit = !(dx * dx + dy * dy > r2);
                if (hit && use_q && (dx != T(0) || dy != T(0))) {
                    // rectangle of offsets [X0, X1] x [Y0, Y1]; minimise q on its four edges
                    const T X0 = x0 - u, X1 = x1 - u, Y0 = y0 - v, Y1 = y1 - v;
                    T qmin = T(3.0e38);
#pragma unroll
                    for (int e = 0; e < 2; e++) {
                        const T X = e ? X1 : X0;            // vertical edges: dy* = b X / a
                        T yy = b_over_a * X;
                        yy = tmin<T>(tmax<T>(yy, Y0), Y1);
                        qmin = tmin<T>(qmin, (c * X * X - T(2) * b * X * yy + a * yy * yy) * rdet);
                        const T Y = e ? Y1 : Y0;            // horizontal edges: dx* = b Y / c
                        T xx = b_over_c * Y;
                        xx = tmin<T>(tmax<T>(xx, X0), X1);
                        qmin = tmin<T>(qmin, (c * xx * xx - T(2) * b * xx * Y + a * Y * Y) * rdet);
                    }
                    hit = !(qmin > tau_m);
                }
                if (hit) touch |= 1u << p;
            }
        }
        const int w = tid >> 6;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const unsigned long long m = __ballot((touch >> p) & 1u);
            if ((tid & 63) == 0) s_mask[p][w] = m;
        }
    }
}

// The same masks for a 64-entry chunk (the fused backward's), by the whole workgroup: wave p tests the 64 staged
// records against patch p -- one patch test per thread instead of four on wave 0 while the other three waves wait at
// the barrier (the masks were 9 % of the backward's wave time, profiles/r04/wave_timeline_D.json).  Every
// (record, patch) pair is tested with the very expressions of build_touch_masks: the same bits.  The records must be
// visible to all waves (barrier after staging).
// (NWORD: the mask words per patch of the caller's array -- 1 at the 64-entry chunk this is for; word 0 is written)
template <int NWORD>
__device__ inline void build_touch_masks_by_patch(const float* s_geom, int cnt, int tid, int tile_x, int tile_y,
                                                  unsigned long long (*s_mask)[NWORD]) {
    const int r = tid & 63, p = tid >> 6;
    bool hit = false;
    if (r < cnt) {
        const float* rec = s_geom + r * GS_PACKED_WIDTH;
        const float u = rec[0], v = rec[1], r2 = rec[2];
        bool use_q = false;
        float a = 0, b = 0, c = 0, rdet = 0, tau_m = 0, b_over_a = 0, b_over_c = 0;
        if (r2 > 0.0f && r2 < 1e30f) {
            a = rec[4]; b = rec[5]; c = rec[6]; rdet = rec[8];
            const float half = 0.5f * (a + c);
            const float lmax = half + fast_sqrt(0.25f * (a - c) * (a - c) + b * b);
            tau_m = (r2 * fast_rcp(lmax)) * 1.001f;
            use_q = a > 0.0f && c > 0.0f && rdet > 0.0f;
            b_over_a = b * fast_rcp(a);
            b_over_c = b * fast_rcp(c);
        }
        const float x0 = float(tile_x * 16 + ((p & 1) << 3)), y0 = float(tile_y * 16 + ((p >> 1) << 3));
        const float x1 = x0 + 7.0f, y1 = y0 + 7.0f;
        float dx = 0.0f, dy = 0.0f;
        if (u < x0) dx = x0 - u;
        if (u > x1) dx = x1 - u;
        if (v < y0) dy = y0 - v;
        if (v > y1) dy = y1 - v;
        hit = !(dx * dx + dy * dy > r2);
        if (hit && use_q && (dx != 0.0f || dy != 0.0f)) {
            const float X0 = x0 - u, X1 = x1 - u, Y0 = y0 - v, Y1 = y1 - v;
            float qmin = 3.0e38f;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const float X = e ? X1 : X0;
                float yy = b_over_a * X;
                yy = tmin(tmax(yy, Y0), Y1);
                qmin = tmin(qmin, (c * X * X - 2.0f * b * X * yy + a * yy * yy) * rdet);
                const float Y = e ? Y1 : Y0;
                float xx = b_over_c * Y;
                xx = tmin(tmax(xx, X0), X1);
                qmin = tmin(qmin, (c * xx * xx - 2.0f * b * xx * Y + a * Y * Y) * rdet);
            }
            hit = !(qmin > tau_m);
        }
    }
    const unsigned long long m = __ballot(hit);
    if (r == 0) s_mask[p][0] = m;
}

// Touch masks handed from the forward to the backward (round 6).  The backward walks the same lists as the forward and
// needs the same (64 entries x 4 patches) touch masks; the forward, which builds them for every chunk it stages, leaves
// the first GS_MASK_WORDS words of every tile behind: touch_masks[(tile * GS_MASK_WORDS + word) * 4 + patch], 512 bytes
// per tile of the GRID (the words beyond -- complete lists walked deeper than 1024 entries -- the backward builds itself).
// Whatever list a tile's final forward pass rendered from (ordered prefix, kept depth prefix, or the complete list of a
// flagged tile's repair pass) is the list its backward walks, and the last pass to render the tile wrote the words.
constexpr int GS_MASK_WORDS = GS_SORT_PREFIX / 64;

// colour of splat i of the staged chunk at this pixel's view direction
template <typename T, int N_SH>
__device__ inline void splat_colour(const T* s_geom, const T* s_col, int i, const T* Y, T* col) {
    if constexpr (N_SH == 1) {
        // sh_to_rgb with one coefficient per channel (spherical_harmonics.cuh:83): the record holds
        // Y0 * coefficient
        const Vec4<T> g2 = *reinterpret_cast<const Vec4<T>*>(s_geom + i * GS_PACKED_WIDTH + 8);
        col[0] = g2.y;
        col[1] = g2.z;
        col[2] = g2.w;
    } else {
        sh_to_rgb<T, N_SH>(s_col + i * ColW<N_SH>::value, Y, col);
    }
}

// ---- software-pipelined LDS record reads (fp32 kernels of the fused renderer) -------------------------
// A wave walking its touch mask is latency-bound, not issue-bound: the wave timeline
// (scripts/render_timeline.py) shows the same ~1200 cycles per visit per wave whether 8 waves or 1 share
// the SIMD, and three dependent LDS round trips (u v r2 | conic, opacity | colour) are a third of it.  The
// whole 48-byte record of the NEXT visit is therefore requested (three ds_read_b128, uniform address)
// before the current visit is worked on, into the other of two register sets.  Volatile loads, so that
// the compiler neither sinks them to their first use nor merges them, pinned by a scheduling barrier; it
// still tracks them, i.e. waits for the current record while the next one is in flight.  Costs 18 VGPRs
// (54 -> 72, 8 -> 7 waves per SIMD) and still wins: forward 0.274 -> 0.265 ms at workload D; prefetching
// only u v r2 opacity | conic (61 VGPRs, 8 waves) and the colour quad at the visit is slower (0.256 vs
// 0.248 ms with the division-free touch masks in both).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const volatile __attribute__((address_space(3))) f32x4* LdsVec4Ptr;
struct LdsRecord {
    f32x4 g0, g1, g2;   // u v r2 opacity | a b c det | 1/det colour
};
__device__ __forceinline__ void lds_record_fetch(LdsRecord& r, const float* rec) {
    LdsVec4Ptr p = (LdsVec4Ptr)(const __attribute__((address_space(3))) float*)rec;
    r.g0 = p[0];
    r.g1 = p[1];
    r.g2 = p[2];
    __builtin_amdgcn_sched_barrier(0);
}

// ---- longest-first tile order for the backward -------------------------------------------------------
// The hardware starts workgroups in grid order and the kernel ends when the last one does; a workgroup
// lives ~150 us of the 520 us backward, so the tail in which the chip drains is a fifth of the kernel
// (scripts/render_timeline.py).  Started longest-first, the tiles that finish last are the short ones.
// The forward measures each tile's own duration (shader clock; the backward of a tile is slow where its
// forward was: same lists, same hit pattern, correlation 0.7) and tile_order_body turns the costs into a
// launch order.  Every XCD keeps its contiguous eighth of the frame (tile_of_block: neighbouring tiles
// add to the same Gaussians' rows, and with one L2 per XCD a frame-wide order doubled the kernel's HBM
// traffic, 194 -> 405 MB): the order is longest-first WITHIN each eighth -- a counting sort on
// 8 x 128 (eighth, cost class) bins -- and block b = 8 j + x starts the j-th tile of eighth x.
// Only the start order changes, no result does.
constexpr int GS_LPT_MIN_TILES = 2048;   // smaller grids: the 6 us of the order kernel exceed the gain
__device__ __forceinline__ void tile_order_body(const int* __restrict__ cost, int tile0, int nt, int n_grid,
                                                int* __restrict__ order) {
    __shared__ int s_hist[1024];
    __shared__ int s_wave[16];
    __shared__ int s_max;
    const int tid = threadIdx.x;
    const int per = n_grid >> 3;   // tiles per XCD (render_grid / tile_of_block)
    s_hist[tid] = 0;
    if (tid == 0) s_max = 1;
    for (int b = tid; b < n_grid; b += 1024) order[b] = -1;
    __syncthreads();
    int mx = 0;
    for (int t = tid; t < nt; t += 1024) mx = max(mx, cost[tile0 + t]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mx = max(mx, __shfl_xor(mx, d));
    if ((tid & 63) == 0) atomicMax(&s_max, mx);
    __syncthreads();
    const float scale = 127.0f / (float)s_max;
    auto bin_of = [&](int t) {   // class 0 = most expensive
        const int c = (int)((float)max(cost[tile0 + t], 0) * scale);
        return (t / per) * 128 + 127 - min(c, 127);
    };
    for (int t = tid; t < nt; t += 1024) atomicAdd(&s_hist[bin_of(t)], 1);
    __syncthreads();
    // exclusive scan of the bin counts: wave scans + one pass over the 16 wave totals
    const int v = s_hist[tid];
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if ((tid & 63) >= d) incl += o;
    }
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    int off = 0;
    for (int w = 0; w < (tid >> 6); w++) off += s_wave[w];
    s_hist[tid] = off + incl - v;
    __syncthreads();
    for (int t = tid; t < nt; t += 1024) {
        const int x = t / per;
        const int rank = atomicAdd(&s_hist[bin_of(t)], 1) - x * per;   // the eighths before x are full
        order[rank * 8 + x] = t;
    }
}

// The backward's prologue, one launch: workgroup 0 makes the launch order (if the tiles are to be started
// longest-first), the others clear the gradient slab the backward accumulates into -- two independent jobs that
// were a 7 us single-workgroup kernel and a 14 us fill one after the other.
constexpr int GS_PROLOGUE_FILL_BLOCKS = 2048;
__global__ __launch_bounds__(1024) void k_bwd_prologue(const int* __restrict__ cost, int tile0, int nt, int n_grid,
                                                       int* __restrict__ order, int ordered, float* __restrict__ slab,
                                                       size_t n_floats) {
    int fill_block = blockIdx.x, fill_blocks = gridDim.x;
    if (order != nullptr) {
        if (blockIdx.x == 0) {
            if (ordered) {
                tile_order_body(cost, tile0, nt, n_grid, order);
            } else {   // (small grids: the natural order, spelled out)
                for (int b = threadIdx.x; b < n_grid; b += 1024) {
                    const int t = tile_of_block(b, nt);
                    order[b] = t < nt ? t : -1;
                }
            }
            return;
        }
        fill_block -= 1;
        fill_blocks -= 1;
    }
    const size_t n4 = n_floats >> 2;   // (the slab is 16-byte aligned: a torch allocation)
    float4* s4 = reinterpret_cast<float4*>(slab);
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (size_t i = (size_t)fill_block * 1024 + threadIdx.x; i < n4; i += (size_t)fill_blocks * 1024) s4[i] = z;
    if (fill_block == 0 && threadIdx.x < (n_floats & 3)) slab[(n4 << 2) + threadIdx.x] = 0.0f;
}

// ---- depth segments of the fused backward ------------------------------------------------------------
// The backward of a tile is a serial walk over its list, back to front; one workgroup per tile lives
// ~150 us, the chip drains for the last fifth of the kernel (4b of DESIGN.md) and a multi-GPU rank's band of
// ~540 tiles is two workgroups per CU.  Splitting the walk by DEPTH gives 3-4x more, 3-4x shorter work
// items -- but a segment that starts in the middle of a pixel's list needs the state the walk would have
// there: the transmittance in front of it and the colour accumulated behind it.  The forward knows both
// and leaves them behind (CK instantiation of the fp32 one-coefficient kernel):
//   per (tile, segment s, pixel)  rec = (P_s, E_s): P_s = product of (1 - alpha) over the segment's contributors,
//                                 E_s = sum of colour * alpha * (product of (1 - alpha) over the segment's EARLIER
//                                 contributors) -- the segment's transmittance and colour as seen from its near
//                                 boundary; 16 bytes, written when the forward crosses into the next segment
//   per pixel                     kend = index after its last contributing splat, and -- evaluated in the
//                                 epilogue for that one splat with the BACKWARD's arithmetic -- 1 - alpha
//                                 and the background weight the backward's first contributor adds
// The backward's walk multiplies weight by 1 / (1 - alpha) per contributor, starting from final_weight (x the
// factor q that render_backward.cu:185 applies -- or not -- at the first contributor, SURVEY.md Q1, which
// then stays in every weight of the walk).  Its weight at the near boundary of segment s' is therefore
//   w(s') = w(s' + 1) / P_s'      from      w(e) = final_weight q (1 - alpha_last) / P_e     (e: the segment
// of the last contributor, whose own factor is in P_e), the colour the walk has accumulated behind segment s is
// bg_weight bg + sum_{s' > s} w(s') E_s', and a workgroup (tile, s) starts every pixel whose list goes deeper
// than its segment from those two; pixels that end inside the segment start as before, pixels that ended in
// front of it do nothing.  (Why products of the (1 - alpha) and not the forward's own transmittance 1 - acc:
// the reference's walk starts from final_weight = 1 - acc of a nearly saturated pixel, whose cancellation error
// -- up to 1e-3 relative -- it carries into every weight of the pixel; a segment that started from the
// forward's accurate 1 - acc at its boundary would be closer to the true derivative and 3e-4 away from the
// reference.  Measured.)
// "Contributor" means: in the BACKWARD's arithmetic -- its alpha differs from the forward's in the last ulp
// and the two can disagree at the 1/255 threshold; the forward evaluates the backward's form where they could
// (see its visit), so the state it leaves describes exactly the walk the unsegmented kernel would do.
#ifndef GS_SEG_LEN
#define GS_SEG_LEN 128
#endif
#ifndef GS_SEG_MAX
#define GS_SEG_MAX 8
#endif
constexpr int SEG_LEN = GS_SEG_LEN;   // entries per segment (a multiple of the 64-entry mask words)
constexpr int SEG_MAX = GS_SEG_MAX;   // segments per tile; the last one is open-ended
static_assert(SEG_LEN % 64 == 0 && SEG_MAX >= 2, "segment geometry");
// the segmented backward walks whole chunks from seg_lo / GS_BWD_CHUNK with no `k >= seg_lo` guard: a segment must
// start on a chunk boundary or its first chunk would re-visit the previous segment's entries
static_assert(SEG_LEN % GS_BWD_CHUNK == 0, "a depth segment must be a whole number of backward chunks");
struct SegState {              // views into the caller's workspace (gs_render_segment_workspace_bytes)
    int* kend;                 // [band pixels], by pixel index - pix0
    float* oma_last;           // same
    float* bgw;                // same
    Vec4<float>* rec;          // [band tiles][SEG_MAX][256], by tile index - tile0
    int tile0;                 // first tile of the band
    int pix0;                  // first pixel of the band
};
constexpr SegState SEG_NONE{nullptr, nullptr, nullptr, nullptr, 0, 0};
// The workspace covers the tile rows [row0, row1) only -- segments are on for bands (a multi-GPU rank's eighth of
// the frame): 32 KB per tile of the BAND, not of the grid (round-3 advisor finding: ~1 GB per frame at 4K to use
// an eighth of it).
__host__ __device__ inline size_t seg_band_pixels(int W, int H, int row0, int row1) {
    const int y0 = row0 * 16 < H ? row0 * 16 : H, y1 = row1 * 16 < H ? row1 * 16 : H;
    return (size_t)W * (size_t)(y1 > y0 ? y1 - y0 : 0);
}
__host__ __device__ inline SegState seg_state_of(void* ws, int W, int H, int row0, int row1) {
    SegState st = SEG_NONE;
    if (ws == nullptr) return st;
    const size_t P = seg_band_pixels(W, H, row0, row1);
    const size_t ntx = (size_t)((W + 15) / 16);
    st.tile0 = (int)ntx * row0;
    st.pix0 = W * (row0 * 16 < H ? row0 * 16 : H);
    char* p = (char*)ws;
    st.rec = (Vec4<float>*)p;   // first: 16-byte aligned
    p += ntx * (size_t)(row1 - row0) * SEG_MAX * 256 * sizeof(Vec4<float>);
    st.kend = (int*)p;
    st.oma_last = (float*)(p + 4 * P);
    st.bgw = (float*)(p + 8 * P);
    return st;
}

// ---------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------
// Two bodies, one tile by one workgroup each: render_tile_fwd_fused (fp32, one colour coefficient: the fused
// renderer's kernels) and render_tile_fwd_general (every other dtype and coefficient count: the reference-shaped
// entry points, gradcheck and the parity tests).  The tile prologue and the pixel epilogue are the same text in both
// (a shared epilogue function changed the register allocation of the four fused kernels: profiles/r10/fwd_split_isa.txt).
//
// The fused renderer's forward.  sort_prefix > 0: prefix mode (binning.hip "prefix sort"), only the
// first sort_prefix entries of a prefix-sorted tile's segment are there; tile_flags[tile] is set to
// whether the tile ran out of them.  flagged_only: the repair call, full list, flags untouched.
// CK: also leaves the state for the depth-segmented backward ("depth segments" above).
template <bool CK>
__device__ __forceinline__ void render_tile_fwd_fused(
    const int tile, const float* __restrict__ packed, const float* __restrict__ rgb,
    const int* __restrict__ ranges, const int* __restrict__ sorted,
    const float* __restrict__ bg, int W, int H, int ntx, int* __restrict__ nsp_out,
    float* __restrict__ fw_out, float* __restrict__ image, int sort_prefix, int* __restrict__ tile_flags,
    bool flagged_only, int64_t cap, int* __restrict__ tile_cost,
    const float* __restrict__ src_opacity, const float* __restrict__ src_conic,
    const SegState seg, const int* __restrict__ full_ranges,
    int* __restrict__ flag_counter, unsigned long long* __restrict__ touch_masks) {
    // the tile's own duration in 16-cycle units: the launch-order key of the backward (tile_order_body)
    const unsigned long long cost_c0 = tile_cost ? __builtin_readcyclecounter() : 0ull;
    constexpr int RCHUNK = Chunk<float, 1>::value;
    __shared__ alignas(16) float s_geom[RCHUNK * GS_PACKED_WIDTH];

    const int tid = threadIdx.x;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    const bool valid = px.u < W && px.v < H;
    const int s0 = ranges[tile];
    const int n_tile = ranges[tile + 1] - s0;
    // lists enqueued with a speculative capacity: a segment beyond it was never written (the caller
    // repeats the frame's binning and this render with the exact size)
    if ((int64_t)s0 + n_tile > cap) {
        if (tile_cost != nullptr && tid == 0) tile_cost[tile] = 0;
        return;
    }
    // prefix mode (binning.hip "prefix sort"): only the first sort_prefix entries are there
    const bool prefix_only = !flagged_only && prefix_sorted_tile(n_tile, sort_prefix);
    const int n_list = prefix_only ? sort_prefix : n_tile;
    // depth cut (binning.hip "depth cut"): `ranges` describe the kept depth prefix of every list, full_ranges the
    // complete ones; a tile whose list was cut short and that reaches its end unsaturated is flagged and redone
    const bool truncated = !flagged_only && full_ranges != nullptr && full_ranges[tile + 1] - full_ranges[tile] > n_tile;

    // A pixel is done when its accumulated alpha exceeds 0.9999 (render.cu:146,162) -- or when it lies outside the
    // image: those lanes start saturated.  "done" is READ OFF acc (one compare per visit) instead of being carried as a
    // flag: the compiler kept the flag as a 0/1 VGPR across the pipelined visits and spent an and, a compare and five
    // moves of every visit's ~52 vector instructions on it.  acc of an outside lane is never used (nothing is stored).
    float acc = valid ? 0.0f : 2.0f, fw = 0;
    auto is_done = [&]() { return acc > Thr<float>::sat_gt(); };
    float img[3] = {0, 0, 0};
    // num_splats_per_pixel == index of the first splat at whose turn the pixel is saturated
    // (render.cu:106,146,162), or the list length: set when the pixel saturates
    int nsp = n_tile;
    const float pu = float(px.u), pv = float(px.v);
    const int wave = tid >> 6;
    constexpr int NW = RCHUNK / 64 > 0 ? RCHUNK / 64 : 1;
    __shared__ unsigned long long s_mask[4][NW];

    // CK: state for the depth-segmented backward (see "depth segments" above)
    float segL = 1;                    // product of (1 - alpha) over the current segment's contributors so far
    float sg0 = 0, sg1 = 0, sg2 = 0;   // sum of colour * alpha * (that product before the splat): the segment's colour
    int kend = 0;                  // index after the last contributing splat
    int b_cur = 0;                 // current segment (wave-uniform)
    bool wave_fin = false;         // the wave's last record is written (every pixel of the patch saturated)
    auto write_record = [&]() {
        if constexpr (CK) {
            Vec4<float> r4;
            r4.x = segL; r4.y = sg0; r4.z = sg1; r4.w = sg2;
            seg.rec[((size_t)(tile - seg.tile0) * SEG_MAX + b_cur) * RB + tid] = r4;
            segL = 1; sg0 = 0; sg1 = 0; sg2 = 0;
        }
    };

    bool all_done = false;
    GS_STAT_DECL;
    GS_HALF_DECL;
    GS_STAT(0, 1);          // waves
    GS_STAT(7, n_tile);     // list entries of the wave's tile
    for (int base = 0; base < n_list; base += RCHUNK) {
        const int cnt = min(RCHUNK, n_list - base);
        GS_STAT(1, 1);      // chunks
        GS_STAT(8, cnt);    // list entries staged
        // TWO_B = 2 / B_DOUBLED: the walk below reads b + b from the record
        stage_chunk<float, 1, 2>(packed, rgb, sorted, s0 + base, cnt, tid, s_geom, nullptr, nullptr, src_opacity, src_conic);
        GS_PHASE(0);
        // (no barrier in between: thread t tests the record thread t staged)
        build_touch_masks<float, RCHUNK, true>(s_geom, cnt, tid, tile % ntx, tile / ntx, s_mask);
        __syncthreads();
        // the chunk's masks for the backward (see GS_MASK_WORDS): thread (word, patch) stores one 8-byte word
        if (touch_masks != nullptr && tid < 4 * NW) {
            const int word = base / 64 + (tid >> 2);
            if (word < GS_MASK_WORDS) touch_masks[((size_t)tile * GS_MASK_WORDS + word) * 4 + (tid & 3)] = s_mask[tid & 3][tid >> 2];
        }
        GS_PHASE(1);
        // pipelined walk: the record of the next visit is in flight while this one is composited
        auto visit = [&](const LdsRecord& r, int i) {
            GS_STAT(2, 1);                              // visits (touch-mask bits walked)
            GS_STAT(6, __popcll(ballot(!is_done())));   // live lanes at the visit
            GS_STAT_FLAG(st_in);
            GS_STAT_FLAG(st_hit);
            if (!is_done()) {
                const float du = pu - r.g0.x, dv = pv - r.g0.y;
                // beyond the cutoff radius alpha < 1/255 is certain: same outcome as render.cu:145-148
                if (!(du * du + dv * dv > r.g0.z)) {
                    GS_STAT_SET(st_in);
                    const float a = r.g1.x, tb = r.g1.y, c = r.g1.z, det = r.g1.w;   // tb = b + b (stage_chunk)
                    const float mh_num = c * du * du - tb * du * dv + a * dv * dv;
                    const float mh = div_by_reciprocal(mh_num, det, r.g2.x);
                    float alpha = r.g0.w * exp_neg_half(mh);
                    // render.cu:133: alpha = 0 unless mh > 0 -- and a zero alpha fails the 1/255 test below.  Without
                    // the segment state only that test reads alpha before it is known to pass: `mh > 0` joins the
                    // test's lane mask (one scalar and) instead of a select in front of it
                    const bool mh_pos = mh > 0.0f;
                    if constexpr (CK) alpha = mh_pos ? alpha : 0.0f;
                    if constexpr (CK) {
                        // What the BACKWARD's walk will see at this entry.  It forms alpha from mh * (1 / det)
                        // (render_backward.cu:153-157; the forward divides), a last-ulp difference that matters
                        // in two places: next to the 1/255 threshold, where the two forms can disagree on whether
                        // the splat contributes at all (~50 (pixel, splat) pairs of a frame at workload D; the
                        // reference's walk then carries one factor 1 / (1 - 1/255) more or less than its forward
                        // did, and so must the segments), and in 1 - alpha for alpha near 1 (6e-8 / (1 - alpha)
                        // relative on the walk's factor).  There the backward's alpha is evaluated as well
                        // (a few percent of the visits); elsewhere the forward's is within 6e-7 of it.
                        // Values for the backward only: contraction allowed.
#pragma clang fp contract(fast)
                        float ab = alpha;
                        const bool near = __builtin_fabsf(alpha - Thr<float>::alpha_min()) < 4e-8f || alpha > 0.9f;
                        if (near) {   // (skipped by the whole wave when no lane is near: s_cbranch_execz)
                            const float mh_b = mh_num * r.g2.x;
                            const float e_b = exp_neg_half(mh_b);
                            ab = r.g0.w * ((mh_b > 0.0f) ? e_b : 0.0f);
                        }
                        // branch-free: a splat the backward skips enters with alpha 0 (changes nothing)
                        const bool cb = ab >= Thr<float>::alpha_min();
                        const float a_cap = Thr<float>::alpha_cap();
                        if (b_cur > 0) {   // (wave-uniform; nobody reads segment 0's record: no segment lies in front of it)
                            const float ac = cb ? ((ab > a_cap) ? a_cap : ab) : 0.0f;   // the backward caps alpha
                            const float aL = ac * segL;
                            sg0 += r.g2.y * aL; sg1 += r.g2.z * aL; sg2 += r.g2.w * aL;
                            segL -= aL;   // segL (1 - ac)
                        }
                        kend = cb ? base + i + 1 : kend;
                    }
                    if (mh_pos & !(alpha < Thr<float>::alpha_min())) {      // render.cu:145
                        GS_STAT_SET(st_hit);
                        // render.cu:149-150: final_weight = 1.0 - acc and weight = alpha * (1.0 - acc), the literal
                        // making both double expressions that are narrowed to float -- six fp64-rate instructions
                        // per contributing visit when written that way.  acc is 0 or >= 1/255 here (it only grows,
                        // and the first weight is an alpha >= 1/255), so 1.0 - (double)acc is EXACT; hence
                        // (a) its narrowing is the correctly rounded float difference, i.e. the float subtraction;
                        // (b) alpha (1 - acc) = alpha - alpha acc as real numbers, and one double fma rounds that
                        // once, exactly as the reference's double multiplication rounds its exact operands.
                        // Same bits, four fp64-rate instructions and one fp32.
                        fw = 1.0f - acc;
                        const float weight = (float)__builtin_fma((double)alpha, -(double)acc, (double)alpha);
                        img[0] += r.g2.y * weight;
                        img[1] += r.g2.z * weight;
                        img[2] += r.g2.w * weight;
                        acc += weight;
                        if (acc > Thr<float>::sat_gt()) {   // saturated: the next splat's check fails
                            nsp = base + i + 1;
                        }
                    }
                }
            }
            GS_STAT(3, ballot(st_in) != 0);           // visits with a lane inside the cutoff circle
            GS_STAT(4, ballot(st_hit) != 0);          // visits with a contributing lane
            GS_STAT(5, __popcll(ballot(st_hit)));     // contributing (pixel, splat) pairs
            GS_HALF_VISIT(ballot(st_in));
        };
        for (int word = 0; word < NW && word * 64 < cnt; word++) {
            if constexpr (CK) {
                // crossing into the next depth segment: leave the state at the boundary behind
                const int sidx = min((base + word * 64) / SEG_LEN, SEG_MAX - 1);
                if (sidx != b_cur && !wave_fin) {
                    write_record();
                    b_cur = sidx;
                }
            }
            if (ballot(!is_done()) == 0) {   // wave-uniform: every pixel of the patch saturated
                if constexpr (CK) {
                    if (!wave_fin) write_record();
                    wave_fin = true;
                }
                break;
            }
            unsigned long long m = wave_uniform(s_mask[wave][word]);
            if (m == 0) continue;
            LdsRecord ra, rb;
            int cur = word * 64 + __builtin_ctzll(m), nxt;
            m &= m - 1;
            lds_record_fetch(ra, s_geom + cur * GS_PACKED_WIDTH);
            while (true) {
                nxt = -1;
                if (m) {
                    nxt = word * 64 + __builtin_ctzll(m);
                    m &= m - 1;
                    lds_record_fetch(rb, s_geom + nxt * GS_PACKED_WIDTH);
                }
                visit(ra, cur);
                if (nxt < 0) break;
                cur = nxt;
                nxt = -1;
                if (m) {
                    nxt = word * 64 + __builtin_ctzll(m);
                    m &= m - 1;
                    lds_record_fetch(ra, s_geom + nxt * GS_PACKED_WIDTH);
                }
                visit(rb, cur);
                if (nxt < 0) break;
                cur = nxt;
            }
        }
        GS_PHASE(2);
        GS_HALF_CHUNK(9);
        all_done = __syncthreads_and(is_done());
        GS_PHASE(3);
        if (all_done) break;
    }
    GS_STAT_FLUSH(0);
    if (tile_cost != nullptr && tid == 0)
        tile_cost[tile] = (int)min((__builtin_readcyclecounter() - cost_c0) >> 4, 0x3fffffffull);
    // an unsaturated pixel at the end of the prefix / of the cut list: the tile is redone from its full list
    if (tile_flags != nullptr && !flagged_only && tid == 0) {
        const bool flag = (prefix_only || truncated) && !all_done;
        tile_flags[tile] = flag;
        if (flag && flag_counter != nullptr) atomicAdd(flag_counter, 1);
    }

    if constexpr (CK) {
        if (!wave_fin) write_record();   // the segment the list (or its ordered prefix) ended in
        if (valid) {
            // the pixel's last contributor once more, in the BACKWARD's arithmetic (k_render_bwd: alpha from
            // mh * (1 / det), capped at 0.9999): what its first step does to weight and colour_accum
            float oma_last = 1, bgw = 0;
            if (kend > 0) {
                const int g = sorted[s0 + kend - 1];
                const Vec4<float>* rec = reinterpret_cast<const Vec4<float>*>(packed + (size_t)g * GS_PACKED_WIDTH);
                const Vec4<float> g0 = rec[0], g1 = rec[1], g2 = rec[2];
                const float du = pu - g0.x, dv = pv - g0.y;
                const float mh = (g1.z * du * du - (g1.y + g1.y) * du * dv + g1.x * dv * dv) * g2.x;
                const float e = exp_neg_half(mh);
                float alpha = g0.w * ((mh > 0.0f) ? e : 0.0f);
                if (alpha > Thr<float>::sat_gt()) alpha = Thr<float>::alpha_cap();
                const float bw = background_weight<float>(alpha, fw);   // render_backward.cu:172-181
                if (bw > Thr<float>::bgw_gt()) bgw = bw;
                oma_last = 1.0f - alpha;
            }
            const size_t p = (size_t)px.v * W + px.u - seg.pix0;
            seg.kend[p] = kend;
            seg.oma_last[p] = oma_last;
            seg.bgw[p] = bgw;
        }
    }
    if (valid) {
        if (acc < Thr<float>::bg_lt()) {   // render.cu:169
#pragma unroll
            for (int ch = 0; ch < 3; ch++) img[ch] += bg[ch] * (1.0 - acc);
        }
        const size_t p = (size_t)px.v * W + px.u;
        nsp_out[p] = nsp;
        fw_out[p] = fw;
        image[p * 3 + 0] = img[0];
        image[p * 3 + 1] = img[1];
        image[p * 3 + 2] = img[2];
    }
}

// The general forward: fp64, and fp32 with per-pixel SH (N_SH > 1: the colour is evaluated from the staged
// coefficients at the pixel's view direction).  Plain walk of the touch masks, one record read per visit; whole
// lists, no flags, no hand-over to a backward.  In fp32 (fast_mode) the cutoff radius and the 1/255 threshold
// skip what cannot contribute; fp64 evaluates every visit as render.cu does.
template <typename T, int N_SH>
__device__ __forceinline__ void render_tile_fwd_general(
    const int tile, const T* __restrict__ packed, const T* __restrict__ rgb,
    const T* __restrict__ view_dir, const int* __restrict__ ranges, const int* __restrict__ sorted,
    const T* __restrict__ bg, int W, int H, int ntx, int* __restrict__ nsp_out,
    T* __restrict__ fw_out, T* __restrict__ image, const T* __restrict__ src_opacity,
    const T* __restrict__ src_conic) {
    static_assert(!(sizeof(T) == 4 && N_SH == 1), "fp32 with one coefficient is render_tile_fwd_fused");
    constexpr int CW = ColW<N_SH>::value;
    constexpr int RCHUNK = Chunk<T, N_SH>::value;
    __shared__ alignas(16) T s_geom[RCHUNK * GS_PACKED_WIDTH];
    __shared__ alignas(16) T s_col[N_SH > 1 ? RCHUNK * CW : 4];

    const int tid = threadIdx.x;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    const bool valid = px.u < W && px.v < H;
    const int s0 = ranges[tile];
    const int n_tile = ranges[tile + 1] - s0;

    T Y[N_SH];
    if constexpr (N_SH > 1) {
        T d[3] = {0, 0, 0};
        if (valid) {
            const T* vd = view_dir + ((size_t)px.v * W + px.u) * 3;
            d[0] = vd[0]; d[1] = vd[1]; d[2] = vd[2];
        }
        sh_basis<T, N_SH>(d, Y);
    } else {
        Y[0] = T(GS_SH_0);
    }

    // A pixel is done when its accumulated alpha exceeds 0.9999 (render.cu:146,162) -- or when it lies outside the
    // image: those lanes start saturated.  acc of an outside lane is never used (nothing is stored).
    T acc = valid ? T(0) : T(2), fw = 0;
    auto is_done = [&]() { return acc > Thr<T>::sat_gt(); };
    T img[3] = {0, 0, 0};
    // num_splats_per_pixel == index of the first splat at whose turn the pixel is saturated
    // (render.cu:106,146,162), or the list length: set when the pixel saturates
    int nsp = n_tile;
    const T pu = T(px.u), pv = T(px.v);
    const int wave = tid >> 6;
    constexpr int NW = RCHUNK / 64 > 0 ? RCHUNK / 64 : 1;
    __shared__ unsigned long long s_mask[4][NW];

    GS_STAT_DECL;
    GS_STAT(0, 1);          // waves
    GS_STAT(7, n_tile);     // list entries of the wave's tile
    for (int base = 0; base < n_tile; base += RCHUNK) {
        const int cnt = min(RCHUNK, n_tile - base);
        GS_STAT(1, 1);      // chunks
        GS_STAT(8, cnt);    // list entries staged
        stage_chunk<T, N_SH>(packed, rgb, sorted, s0 + base, cnt, tid, s_geom, s_col, nullptr, src_opacity, src_conic);
        GS_PHASE(0);
        // (no barrier in between: thread t tests the record thread t staged)
        build_touch_masks<T, RCHUNK>(s_geom, cnt, tid, tile % ntx, tile / ntx, s_mask);
        __syncthreads();
        GS_PHASE(1);
        for (int word = 0; word < NW && word * 64 < cnt; word++) {
            if (ballot(!is_done()) == 0) break;   // wave-uniform: every pixel of the patch saturated
            unsigned long long m = wave_uniform(s_mask[wave][word]);
            while (m) {
                const int i = word * 64 + __builtin_ctzll(m);
                m &= m - 1;
                GS_STAT(2, 1);                        // visits (touch-mask bits walked)
                GS_STAT(6, __popcll(ballot(!is_done())));   // live lanes at the visit
                GS_STAT_FLAG(st_in);
                GS_STAT_FLAG(st_hit);
                if (!is_done()) {
                    const T* rec = s_geom + i * GS_PACKED_WIDTH;
                    const Vec4<T> g0 = *reinterpret_cast<const Vec4<T>*>(rec);   // u v r2 opacity
                    const T du = pu - g0.x, dv = pv - g0.y;
                    // beyond the cutoff radius alpha < 1/255 is certain: same outcome as :145-148
                    if (!(fast_mode<T>() && du * du + dv * dv > g0.z)) {
                        GS_STAT_SET(st_in);
                        const Vec4<T> g1 = *reinterpret_cast<const Vec4<T>*>(rec + 4);   // a b c det
                        const Vec4<T> g2 = *reinterpret_cast<const Vec4<T>*>(rec + 8);   // 1/det, colour
                        const T a = g1.x, b = g1.y, c = g1.z, det = g1.w;
                        const T mh = div_by_reciprocal(c * du * du - (b + b) * du * dv + a * dv * dv, det, g2.x);
                        T alpha = g0.w * exp_neg_half(mh);
                        alpha = (mh > T(0)) ? alpha : T(0);                 // render.cu:133
                        if (!(fast_mode<T>() && alpha < Thr<T>::alpha_min())) {       // render.cu:145
                            GS_STAT_SET(st_hit);
                            fw = 1.0 - acc;
                            const T weight = alpha * (1.0 - acc);           // double, narrowed
                            T col[3];
                            splat_colour<T, N_SH>(s_geom, s_col, i, Y, col);
#pragma unroll
                            for (int ch = 0; ch < 3; ch++) img[ch] += col[ch] * weight;
                            acc += weight;
                            if (acc > Thr<T>::sat_gt()) {   // saturated: the next splat's check fails
                                nsp = base + i + 1;
                            }
                        }
                    }
                }
                GS_STAT(3, ballot(st_in) != 0);           // visits with a lane inside the cutoff circle
                GS_STAT(4, ballot(st_hit) != 0);          // visits with a contributing lane
                GS_STAT(5, __popcll(ballot(st_hit)));     // contributing (pixel, splat) pairs
            }
        }
        GS_PHASE(2);
        const bool all_done = __syncthreads_and(is_done());
        GS_PHASE(3);
        if (all_done) break;
    }
    GS_STAT_FLUSH(0);

    if (valid) {
        if (acc < Thr<T>::bg_lt()) {   // render.cu:169
#pragma unroll
            for (int ch = 0; ch < 3; ch++) img[ch] += bg[ch] * (1.0 - acc);
        }
        const size_t p = (size_t)px.v * W + px.u;
        nsp_out[p] = nsp;
        fw_out[p] = fw;
        image[p * 3 + 0] = img[0];
        image[p * 3 + 1] = img[1];
        image[p * 3 + 2] = img[2];
    }
}

// the fused renderer's forward: whole frame, prefix mode or depth-cut lists.  (The parameter list is the one every
// fp32 / fp64, 1..16-coefficient forward had while they were one kernel: view_dir is unused.)
template <typename T, int N_SH>
__global__ __launch_bounds__(RB) void k_render_fwd(
    const T* __restrict__ packed, const T* __restrict__ rgb, const T* __restrict__ view_dir,
    const int* __restrict__ ranges, const int* __restrict__ sorted, const T* __restrict__ bg,
    int W, int H, int ntx, int tile0, int nt, int* __restrict__ nsp_out, T* __restrict__ fw_out,
    T* __restrict__ image, int sort_prefix, int* __restrict__ tile_flags, int64_t cap,
    int* __restrict__ tile_cost, const T* __restrict__ src_opacity, const T* __restrict__ src_conic,
    const int* __restrict__ full_ranges, int* __restrict__ flag_counter, unsigned long long* __restrict__ touch_masks) {
    static_assert(sizeof(T) == 4 && N_SH == 1, "the fused fp32 kernel; everything else goes to k_render_fwd_general");
    const int t_local = tile_of_block(blockIdx.x, nt);
    if (t_local >= nt) return;
    // Launch position sets the wave priority: the last eighth of the grid runs at priority 1.  A SIMD arbitrates
    // vector issue by priority, then age, so the workgroups dispatched last -- whose completion ends the kernel --
    // would otherwise be the losers on every SIMD they share with older tiles (profiles/r15/render_wave_priority_ab.txt).
    // Block index and a kernel argument only: a scalar compare and branch around one s_setprio, which ignores EXEC.
    {
        const int grid = (nt + 7) & ~7;   // render_grid(nt)
        if ((int)blockIdx.x >= grid - (grid >> 3)) __builtin_amdgcn_s_setprio(1);
    }
    render_tile_fwd_fused<false>(tile0 + t_local, packed, rgb, ranges, sorted, bg, W, H, ntx,
                                 nsp_out, fw_out, image, sort_prefix, tile_flags, false, cap, tile_cost, src_opacity,
                                 src_conic, SEG_NONE, full_ranges, flag_counter, touch_masks);
}

template <typename T, int N_SH>
__global__ __launch_bounds__(RB) void k_render_fwd_general(
    const T* __restrict__ packed, const T* __restrict__ rgb, const T* __restrict__ view_dir,
    const int* __restrict__ ranges, const int* __restrict__ sorted, const T* __restrict__ bg,
    int W, int H, int ntx, int tile0, int nt, int* __restrict__ nsp_out, T* __restrict__ fw_out,
    T* __restrict__ image, const T* __restrict__ src_opacity, const T* __restrict__ src_conic) {
    const int t_local = tile_of_block(blockIdx.x, nt);
    if (t_local >= nt) return;
    render_tile_fwd_general<T, N_SH>(tile0 + t_local, packed, rgb, view_dir, ranges, sorted, bg, W, H, ntx,
                                     nsp_out, fw_out, image, src_opacity, src_conic);
}

// the fused renderer's forward that also leaves the state for the depth-segmented backward
#ifndef GS_FWD_CK_WAVES
#define GS_FWD_CK_WAVES 5   // no spills at 5 (90 VGPRs); the kernel runs where a band leaves 2-3 waves per SIMD anyway
#endif
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(GS_FWD_CK_WAVES, 8))) void k_render_fwd_ck(
    const float* __restrict__ packed, const float* __restrict__ rgb, const int* __restrict__ ranges,
    const int* __restrict__ sorted, const float* __restrict__ bg, int W, int H, int ntx, int tile0, int nt,
    int* __restrict__ nsp_out, float* __restrict__ fw_out, float* __restrict__ image, int sort_prefix,
    int* __restrict__ tile_flags, int64_t cap, int* __restrict__ tile_cost, const SegState seg,
    unsigned long long* __restrict__ touch_masks) {
    const int t_local = tile_of_block(blockIdx.x, nt);
    if (t_local >= nt) return;
    render_tile_fwd_fused<true>(tile0 + t_local, packed, rgb, ranges, sorted, bg, W, H, ntx, nsp_out,
                                fw_out, image, sort_prefix, tile_flags, false, cap, tile_cost, nullptr, nullptr,
                                seg, nullptr, nullptr, touch_masks);
}

// repair pass of the prefix mode / of the depth cut, ONE launch: a small grid walks the flags; a flagged tile's list is
// first sorted in full by the workgroup (sort_keys != nullptr: lists up to SORT_MAX_LDS_KEYS entries in LDS, longer
// ones -- sort_beyond -- in global memory; in prefix mode, sort_prefix > 0, only the lists that were prefix-sorted need
// it) and then rendered again from it.  (Two launches until round 5 -- a sort kernel and this one: ~5 us each on the
// frames where no tile is flagged, which is nearly all of them.)
template <bool CK>
__global__ __launch_bounds__(RB) __attribute__((amdgpu_waves_per_eu(GS_FWD_CK_WAVES, 8))) void k_render_fwd_flagged(
    const float* __restrict__ packed, const float* __restrict__ rgb, const int* __restrict__ ranges,
    int* __restrict__ sorted, const float* __restrict__ bg, int W, int H, int ntx, int tile0,
    int nt, int* __restrict__ nsp_out, float* __restrict__ fw_out, float* __restrict__ image,
    int* __restrict__ tile_flags, int64_t cap, int* __restrict__ tile_cost, const SegState seg,
    const int* __restrict__ flag_counter, int* __restrict__ host_flagged, uint64_t* __restrict__ sort_keys,
    int sort_prefix, int sort_beyond, unsigned long long* __restrict__ touch_masks) {
    extern __shared__ uint64_t s_sort_keys[];
    static_assert(RB == SORT_BLOCK, "the repair workgroup sorts with the binning's network");
    // (depth cut) how many tiles of the frame had to be repaired, into the caller's pinned host word: what the
    // orchestration's policy looks at before later frames (never waited for)
    if (host_flagged != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *host_flagged = *flag_counter;
    if (flag_counter != nullptr && *flag_counter == 0) return;   // (depth cut: no tile of the frame is flagged)
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < nt; t += gridDim.x) {
        const int tile = tile0 + t;
        if (tile_flags[tile] == 0) continue;
        if (sort_keys != nullptr) {
            const int s0 = ranges[tile];
            const int n = ranges[tile + 1] - s0;
            const bool wanted = sort_prefix > 0 ? prefix_sorted_tile(n, sort_prefix) : n > 1;
            if (wanted && (int64_t)s0 + n <= cap) {   // (block-uniform)
                if (n <= SORT_MAX_LDS_KEYS) {
                    for (int i = tid; i < n; i += SORT_BLOCK) s_sort_keys[slot(i)] = sort_keys[s0 + i];
                    __syncthreads();
                    lds_bitonic_sort(s_sort_keys, n, tid);
                    for (int i = tid; i < n; i += SORT_BLOCK) sorted[s0 + i] = (int)(uint32_t)s_sort_keys[slot(i)];
                } else if (sort_beyond) {
                    global_sort_tile(sort_keys + s0, sorted + s0, n, tid);
                }
            }
            __syncthreads();   // the list is in place for every thread of the workgroup (workgroup-scope fence + barrier)
        }
        render_tile_fwd_fused<CK>(tile, packed, rgb, ranges, sorted, bg, W, H, ntx,
                                  nsp_out, fw_out, image, 0, tile_flags, true, cap, tile_cost, nullptr, nullptr,
                                  seg, nullptr, nullptr, touch_masks);
        __syncthreads();
    }
}
// the repair kernel's dynamic LDS (the sort's keys): the limit is raised once per device
template <bool CK> static void repair_attr_once() {
    static std::atomic<uint64_t> seen{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    const uint64_t bit = 1ull << dev;
    if ((seen.fetch_or(bit) & bit) == 0)
        (void)hipFuncSetAttribute((const void*)k_render_fwd_flagged<CK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)sort_lds_bytes(SORT_MAX_LDS_KEYS));
}
// the repair launch: at most 512 workgroups walk the flags of the nt tiles from tile0 on, `lds` bytes for the sort
template <bool CK>
static void launch_render_fwd_flagged(
    hipStream_t s, size_t lds, const void* packed, const void* rgb, const int* ranges, int* sorted, const void* bg, int W,
    int H, int ntx, int tile0, int nt, int* nsp_out, void* fw_out, void* image, int* tile_flags, int64_t cap,
    int* tile_cost, const SegState seg, const int* flag_counter, int* host_flagged, uint64_t* sort_keys,
    int sort_prefix, int sort_beyond, uint64_t* touch_masks) {
    repair_attr_once<CK>();
    k_render_fwd_flagged<CK><<<nt < 512 ? nt : 512, RB, lds, s>>>(
        (const float*)packed, (const float*)rgb, ranges, sorted, (const float*)bg, W, H, ntx, tile0, nt, nsp_out,
        (float*)fw_out, (float*)image, tile_flags, cap, tile_cost, seg, flag_counter, host_flagged, sort_keys,
        sort_prefix, sort_beyond, (unsigned long long*)touch_masks);
}

// ---------------------------------------------------------------------------------------------------
// wave reductions
// ---------------------------------------------------------------------------------------------------
// Sum over the 64 lanes, result valid in lane 63 (the fp64 reference backward: plain shuffles).
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d);
        if ((int)(threadIdx.x & 63) >= d) v += o;
    }
    return v;
}

template <typename T> __device__ inline void global_add(T* p, T v) { unsafeAtomicAdd(p, v); }


// v_permlane16_swap_b32 a, b: rows 1 and 3 (16-lane rows) of a are exchanged with rows 0 and 2 of b;
// v_permlane32_swap_b32 a, b: lanes 32..63 of a with lanes 0..31 of b (gfx950).  Inline assembly: this
// toolchain's builtin hands back its first result twice (scripts/ubench/permlane_test.hip checks the
// semantics on the device).  Must run with all 64 lanes enabled.
__device__ __forceinline__ void permlane16_swap(float& a, float& b) {
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void permlane32_swap(float& a, float& b) {
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}

// A DPP move as a value (the compiler folds it into the add behind it and pads the read-after-write hazard itself).
template <int CTRL>
__device__ __forceinline__ unsigned dpp_lanes(unsigned x) {   // x of the lane the DPP control names (all of them in range)
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_lanes(float x) { return __uint_as_float(dpp_lanes<CTRL>(__float_as_uint(x))); }

// Sums TWO per-lane values over the wave (the absgrad pair of k_render_bwd_abs; k_render_contrib's exchange
// with two sums): four DPP steps inside the 16-lane rows (xor 1, xor 2, row_ror 4, row_ror 8: every lane holds its
// row's total), permlane16_swap pairs the rows -- a's row pairs (0,1), (2,3) land in rows 0, 2, b's in rows 1, 3 --
// and permlane32_swap joins the halves: lane 0 ends with a's total, lane 16 with b's, (r0 + r1) + (r2 + r3) in a
// fixed order.  Those two lanes store with one ds_write_b32 (pair_slot: the wave's pair of this splat + lane / 16).
// Lanes that do not contribute must hold zeros; all 64 lanes must be enabled.
__device__ __forceinline__ void reduce2_to_slot(float a, float b, bool stores, float* slots, int pair_slot) {
    a += dpp_lanes<0xB1>(a);  b += dpp_lanes<0xB1>(b);     // quad_perm [1,0,3,2]
    a += dpp_lanes<0x4E>(a);  b += dpp_lanes<0x4E>(b);     // quad_perm [2,3,0,1]
    a += dpp_lanes<0x124>(a); b += dpp_lanes<0x124>(b);    // row_ror:4
    a += dpp_lanes<0x128>(a); b += dpp_lanes<0x128>(b);    // row_ror:8
    permlane16_swap(a, b);           // a: rows (a0, b0, a2, b2); b: rows (a1, b1, a3, b3)
    float z = a + b;
    float z2 = z;
    permlane32_swap(z, z2);          // z: rows 0, 1 twice; z2: rows 2, 3 twice
    const float total = z + z2;
    if (stores) slots[pair_slot] = total;
}

// Sums nine per-lane values over the 64 lanes of the wave and stores the nine totals to slot[0..8]
// (LDS, owned by this wave for this splat: plain stores, no atomics -- an LDS float atomic costs
// ~3.5 cycles PER ACTIVE LANE on gfx950, which made the accumulators the bound of the kernel).
// A TRANSPOSING reduction: instead of summing all 9 values in every lane (54 cross-lane adds), lanes
// trade halves of the value set -- after the stride-4 step a lane keeps 4 of the first 8 values, after the
// stride-8 step 2 (see the function body) -- one v_permlane16_swap puts the even values' row pairs in
// rows 0/2 and the odd values' in rows 1/3, one v_permlane32_swap joins the halves: totals of the even
// values end in row 0, of the odd values in row 1, the ninth in lanes 48..63 (rows 1 + 3, joined by a row_bcast:15 add); nine lanes store with
// ONE ds_write_b32 (slot_lane_offset gives each its element, -1 elsewhere).
// Lanes that do not contribute must hold zeros.
__device__ __forceinline__ int slot_lane_offset(int lane) {
    // after the reduction: row 0 holds the totals of the even values, row 1 of the odd ones, bank k of a
    // row (lanes 4k..4k+3) the pair e(k) = (0, 4, 2, 6)[k]; lanes 48..63 hold the ninth value (lane 63 stores it)
    if (lane == 63) return 8;
    if (lane >= 32 || (lane & 3) != 0) return -1;
    const int bank = (lane >> 2) & 3;
    const int e = ((bank & 1) ? 4 : 0) + ((bank & 2) ? 2 : 0);
    return lane < 16 ? e : e + 1;
}
__device__ __forceinline__ void reduce9_to_slot(const float* val, bool stores, float* slots, int lane_slot) {
    // Rows first (16 lanes), hand-scheduled.  A DPP add with a BANK mask writes only the enabled quads
    // (bank = the four lanes i/4 of a row), so the trade "keep one half of the values, send the other"
    // needs no select when it is done ACROSS quads:
    //   stride 4   r_j = banks 0,2: v_j + v_j@(i+4)          banks 1,3: v_{j+4} + v_{j+4}@(i-4)     (j = 0..3)
    //   stride 8   s_j = banks 0,1: r_j + r_j@(i+8)          banks 2,3: r_{j+2} + r_{j+2}@(i-8)     (j = 0, 1)
    //   inside the quads the two survivors are summed plainly (xor 1, xor 2): every lane of bank k then
    //   holds the ROW totals of values e(k), e(k)+1 with e = (0, 4, 2, 6); the ninth value takes xor 1,
    //   xor 2, row_ror 12, row_ror 8 (row total in every lane).
    // 20 DPP adds and no v_cndmask (the compiler's form of the same trade: 12 selects + 17 DPP ops).
    // Every DPP source was written at least two instructions earlier (the DPP read-after-VALU-write hazard
    // needs two wait states; the s_nop covers the compiler's code in front of the block).
    float r0, r1, r2, r3, s2[2], s8;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %7, %7 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %1, %8, %8 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %2, %9, %9 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %3, %10, %10 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %0, %11, %11 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %1, %12, %12 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %2, %13, %13 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %3, %14, %14 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %6, %15, %15 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %4, %0, %0 row_shl:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %5, %1, %1 row_shl:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %4, %2, %2 row_shr:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %5, %3, %3 row_shr:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %6, %6, %6 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %4, %4, %4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %5, %5, %5 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %6, %6, %6 row_ror:12 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %4, %4, %4 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %5, %5, %5 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %6, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(s2[0]), "=&v"(s2[1]), "=&v"(s8)
        : "v"(val[0]), "v"(val[1]), "v"(val[2]), "v"(val[3]), "v"(val[4]), "v"(val[5]), "v"(val[6]), "v"(val[7]),
          "v"(val[8]));
    // rows -> wave
    float x = s2[0], y = s2[1];
    permlane16_swap(x, y);           // x: rows (x0, y0, x2, y2); y: rows (x1, y1, x3, y3)
    float z = x + y;                 // rows 0, 2: even values of row pairs (0,1), (2,3); rows 1, 3: odd values
    // ninth value (its row total in every lane): rows 1 and 3 add lane 15 of the row in front of them (DPP row_bcast:15)
    // -- rows 0+1 and 2+3 as the two-register lane swap + add formed them, for one DPP add instead of a move, an
    // 8-cycle swap with its hazard padding and an add.  Lane 63 stores it: with the third step of the row reduction
    // rotating by 12 (quad q + quad q+1) lane 15 of every row holds ((Q3+Q0)+(Q1+Q2)), bit for bit the association
    // lane 0 held -- and lane 32 stored -- when that step rotated by 4
    float e = s8;
    asm volatile("v_add_f32_dpp %0, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 0" : "+v"(e) : "v"(s8));
    permlane32_swap(z, e);           // z: (z.lo, e.lo); e: (z.hi, e.hi)
    const float total = z + e;       // lanes 0..31: even / odd values' totals; lanes 48..63: the ninth (rows 0+1 + rows 2+3)
    // (lane_slot: the wave's slot of this splat + slot_lane_offset(lane), formed by the caller from a per-lane base that
    // holds everything but the splat -- one vector add per visit where (wave, splat, lane) -> address took three)
    if (stores) slots[lane_slot] = total;
}

// Phase 1 of the flush of k_render_bwd_sh and of the map walk (k_render_bwd has the same text written out, see there;
// one global atomic per value per (splat, tile)), thread = staged splat: add the slots of the waves that wrote this
// splat (s_hit [wave][RCHUNK / 64 words]), in wave order (deterministic per tile), apply the per-splat factors -- the
// sums of (w, w du, w dv) and of the per-pixel conic terms become gradients with k = -0.5 opacity / det -- and park
// the row in wave 0's slot of the same splat.  Each thread only ever touches its own splat's slots: no barrier needed
// before; the caller puts one behind, in front of its Phase 2.
template <int RCHUNK, int SV>
__device__ __forceinline__ void flush_sum_slots(float* s_acc, const float* s_geom,
                                                const unsigned long long (*s_hit)[RCHUNK / 64 > 0 ? RCHUNK / 64 : 1],
                                                int tid, int cnt) {
    if (tid < cnt) {
        float a[SV];
#pragma unroll
        for (int j = 0; j < SV; j++) a[j] = 0;
        bool any_hit = false;
#pragma unroll
        for (int w4 = 0; w4 < 4; w4++) {
            if ((s_hit[w4][tid >> 6] >> (tid & 63)) & 1ull) {
                any_hit = true;
                const float* sl = s_acc + (w4 * RCHUNK + tid) * SV;
#pragma unroll
                for (int j = 0; j < SV; j++) a[j] += sl[j];
            }
        }
        // (a splat no wave hit keeps its zeros unscaled: 1 / det = inf of a record whose determinant cancelled to 0
        // would make them NaN; see render_bwd_walk.inc)
        const float* rec = s_geom + tid * GS_PACKED_WIDTH;
        const float ca = rec[4], cb = rec[5], cc = rec[6];
        const float k = any_hit ? -0.5f * rec[3] * rec[8] : 0.0f;
        const float Mu = a[4], Mv = a[5];
        a[4] = -2.0f * k * (cc * Mu - cb * Mv);
        a[5] = -2.0f * k * (ca * Mv - cb * Mu);
        a[6] *= k;
        a[7] *= k;
        a[8] *= k;
        float* row = s_acc + tid * SV;
#pragma unroll
        for (int j = 0; j < SV; j++) row[j] = a[j];
    }
}

// ---------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------
// The fp32 kernels.  At most 7 waves per SIMD (no minimum: k_render_bwd_sh sits far below).  Squeezed into the 64
// registers of 8 waves, k_render_bwd<float, 1> reloads a coefficient of the exponential in every visit; with the 72
// of 7 it stays resident (104 -> 103 vector instructions per visit, 0.4506 -> 0.4466 ms at D alternating on one box),
// and the kernel never held 8 waves anyway (5-7).  Among those 5-7 waves the position in the list sets the
// wave priority (the chunk loop of k_render_bwd<float, 1>): a wave deep in its list goes first.
#ifdef GS_BWD_WAVES
#define GS_BWD_OCC __attribute__((amdgpu_waves_per_eu(GS_BWD_WAVES, GS_BWD_WAVES)))
#else
#define GS_BWD_OCC __attribute__((amdgpu_waves_per_eu(1, 7)))
#endif
//
// k_render_bwd<float, 1>: the fused renderer's backward, fp32 with one colour coefficient per channel (the record's
// colour is Y0 * coefficient; per-pixel SH is k_render_bwd_sh, fp64 k_render_bwd_ref).  Three launches:
//   launch_render_bwd (gs_render_tiles_backward / _packed, float32, n_sh == 1): whole lists in grid order into the four
//     separate gradient arrays (slab == 0), records staged from packed ones or from the reference's separate arrays
//     (src_opacity / src_conic);
//   gs_render_tiles_backward_slab: into the [V, 9] slab, tiles in tile_order (longest first) when given, depth-cut
//     overflow lists and handed-over touch masks when given;
//   the same with segment_state: work items (tile, depth segment), each resuming the pixels' walks from the state the
//     forward left (SegState).
// The template header and the full parameter list (view_dir: unused) are kept: profiles and scripts know the kernel
// under this name, and its argument layout is the one they recorded.
//
// The walk is ONE text, render_bwd_walk.inc, included by two kernels: k_render_bwd<float, 1> (GS_BWD_ABS 0: the tokens
// and the instructions the kernel has always had -- scripts/kernel_isa_diff.py, profiles/r16/absgrad_isa.txt) and
// k_render_bwd_abs (GS_BWD_ABS 1, the slab form only, behind gs_render_tiles_backward_slab_abs), which next to the
// nine sums accumulates the per-pixel MAGNITUDES of the uv gradient's terms (AbsGS):
//   visit   e_u = |wz (c du - b dv)|, e_v = |wz (a dv - b du)| -- expressions of their own, outside the contraction
//           blocks, so that no instruction of the nine sums depends on them; 0 in lanes that do not contribute
//   wave    reduce2_to_slot into the wave's own pair per staged splat (s_abs [wave][splat][2], 2 KB; reduce9_to_slot
//           and the nine-word slots stay as they are), in the visits that write the nine-word slot (s_hit serves both)
//   flush   thread = splat adds the pairs of the waves that wrote, multiplies by opacity |1 / det| (rec[3] |rec[8]| = |-2k|
//           of the nine sums' flush) and parks the pair in wave 0's; a second short pass, thread = value, sends one
//           global atomic per value per (splat, tile) to g_uv_abs[g, 2]; rows of two zeros stay untouched
template <typename T, int N_SH>
__global__ __launch_bounds__(RB) GS_BWD_OCC void k_render_bwd(
    const T* __restrict__ packed, const T* __restrict__ rgb, const T* __restrict__ view_dir,
    const int* __restrict__ ranges, const int* __restrict__ sorted, const T* __restrict__ bg,
    const int* __restrict__ nsp_in, const T* __restrict__ fw_in, const T* __restrict__ grad_image,
    int W, int H, int ntx, int tile0, int nt, T* __restrict__ g_rgb, T* __restrict__ g_opa,
    T* __restrict__ g_uv, T* __restrict__ g_conic, int slab, int exact, const int* __restrict__ tile_order,
    const T* __restrict__ src_opacity, const T* __restrict__ src_conic, const SegState seg,
    const int* __restrict__ cut_flags, const int* __restrict__ full_ranges, const int* __restrict__ overflow_sorted,
    const unsigned long long* __restrict__ touch_masks) {
    static_assert(sizeof(T) == 4 && N_SH == 1, "the fused fp32 kernel; per-pixel SH goes to k_render_bwd_sh, fp64 to k_render_bwd_ref");
#define GS_BWD_ABS 0
#include "render_bwd_walk.inc"
#undef GS_BWD_ABS
}

// The absgrad form (gs_render_tiles_backward_slab_abs): the same parameters and g_uv_abs[V, 2] behind them.  Launched
// in the slab forms only (slab = 1, g_opa = g_uv = g_conic = src_opacity = src_conic = NULL).
__global__ __launch_bounds__(RB) GS_BWD_OCC void k_render_bwd_abs(
    const float* __restrict__ packed, const float* __restrict__ rgb, const float* __restrict__ view_dir,
    const int* __restrict__ ranges, const int* __restrict__ sorted, const float* __restrict__ bg,
    const int* __restrict__ nsp_in, const float* __restrict__ fw_in, const float* __restrict__ grad_image,
    int W, int H, int ntx, int tile0, int nt, float* __restrict__ g_rgb, float* __restrict__ g_opa,
    float* __restrict__ g_uv, float* __restrict__ g_conic, int slab, int exact, const int* __restrict__ tile_order,
    const float* __restrict__ src_opacity, const float* __restrict__ src_conic, const SegState seg,
    const int* __restrict__ cut_flags, const int* __restrict__ full_ranges, const int* __restrict__ overflow_sorted,
    const unsigned long long* __restrict__ touch_masks,
    float* __restrict__ g_uv_abs) {
#define GS_BWD_ABS 1
#include "render_bwd_walk.inc"
#undef GS_BWD_ABS
}

// The fp32 backward with per-pixel SH (N_SH = 4 / 9 / 16 coefficients per channel; render_backward.cu:422-488), behind
// gs_render_tiles_backward / _packed only: launch_render_bwd is its one caller.  The same walk as k_render_bwd --
// chunks of GS_BWD_CHUNK from the tile's deepest used splat to the front, touch masks built here, Q1, the wave's slot
// per staged splat, the two-phase flush -- over whole lists and into the four separate gradient arrays: no slab, tile
// order, depth segments, depth-cut lists or handed-over masks.  A splat's colour is evaluated at the pixel's view
// direction from the staged coefficients (s_col), and the colour-coefficient gradients leave the slots: the gradient
// of coefficient (ch, s) of a splat is sum over pixels of Y_s(p) gi_ch(p) * aw(p), a contraction over the wave's 64
// pixels whose left factor does not depend on the splat -- a GEMM [16 x 64] x [64 x 16 splats] per channel, done with
// v_mfma_f32_16x16x4_f32 (exact fp32) on batches of 16 contributing splats instead of 3 * N_SH cross-lane reductions
// per visit.  The slot stays nine wide with its three colour sums unused: a six-value reduction would change the
// kernel's speed, which the split that gave it a body of its own did not set out to do.
template <int N_SH>
__global__ __launch_bounds__(RB) GS_BWD_OCC void k_render_bwd_sh(
    const float* __restrict__ packed, const float* __restrict__ rgb, const float* __restrict__ view_dir,
    const int* __restrict__ ranges, const int* __restrict__ sorted, const float* __restrict__ bg,
    const int* __restrict__ nsp_in, const float* __restrict__ fw_in, const float* __restrict__ grad_image,
    int W, int H, int ntx, int tile0, int nt, float* __restrict__ g_rgb, float* __restrict__ g_opa,
    float* __restrict__ g_uv, float* __restrict__ g_conic, int exact, const float* __restrict__ src_opacity,
    const float* __restrict__ src_conic) {
    static_assert(N_SH > 1, "per-pixel SH; one coefficient goes to k_render_bwd<float, 1>");
    constexpr int CW = ColW<N_SH>::value;
    constexpr int C = 3 * N_SH;
    constexpr int REF_CH = ref_chunk<float>(N_SH);
    constexpr int SV = 9;   // width of a slot: colour 3 (unused) | w, w du, w dv | conic terms 3
    constexpr int RCHUNK = GS_BWD_CHUNK;
    constexpr int NWORD = RCHUNK / 64 > 0 ? RCHUNK / 64 : 1;
    constexpr int MB = 16;        // splats per MFMA batch (the N of 16x16x4)
    constexpr int BROW = 64 + 4;  // floats per row of the batch's aw matrix [slot][pixel] (16-byte aligned rows)
    __shared__ alignas(16) float s_geom[RCHUNK * GS_PACKED_WIDTH];
    __shared__ alignas(16) float s_col[RCHUNK * CW];
    __shared__ int s_idx[RCHUNK];
    __shared__ float s_acc[4 * RCHUNK * SV];              // [wave][splat][9]
    __shared__ alignas(16) float s_B[4 * MB * BROW];      // [wave][slot][pixel] aw of the open batch
    __shared__ int s_bidx[4 * MB];                         // [wave][slot] Gaussian index of the splat
    __shared__ alignas(16) float s_gi[4 * 3 * 64];        // [wave][ch][pixel] grad_image
    __shared__ int s_max[4];
    __shared__ unsigned long long s_mask[4][NWORD];
    __shared__ unsigned long long s_hit[4][NWORD];        // slots written by each wave

    const int t_local = tile_of_block(blockIdx.x, nt);
    if (t_local >= nt) return;
    const int tile = tile0 + t_local;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    const bool valid = px.u < W && px.v < H;
    const int s0 = ranges[tile];
    const int n_tile = ranges[tile + 1] - s0;
    if (n_tile <= 0) return;

    int nsp = 0;
    float weight = 0;
    float gi[3] = {0, 0, 0};
    float Y[N_SH];
    {
        float d[3] = {0, 0, 0};
        if (valid) {
            const size_t p = (size_t)px.v * W + px.u;
            nsp = nsp_in[p];
            weight = fw_in[p];
            gi[0] = grad_image[p * 3 + 0];
            gi[1] = grad_image[p * 3 + 1];
            gi[2] = grad_image[p * 3 + 2];
            d[0] = view_dir[p * 3 + 0]; d[1] = view_dir[p * 3 + 1]; d[2] = view_dir[p * 3 + 2];
        }
        sh_basis<float, N_SH>(d, Y);
    }
    // the tile's deepest used splat (render_backward.cu:131 makes everything beyond it a no-op)
    int m = nsp;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, __shfl_xor(m, d));
    if (lane == 0) s_max[wave] = m;
    __syncthreads();
    const int n_used = min(n_tile, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
    if (n_used <= 0) return;

    const float pu = float(px.u), pv = float(px.v);
    const int slot_off = slot_lane_offset(lane);
    const bool slot_stores = slot_off >= 0;
    const int slot_lane_base = wave * RCHUNK * SV + (slot_stores ? slot_off : 0);
    float color_accum[3] = {0, 0, 0};
    bool bg_init = false;
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];

    // The batch GEMM, per channel  D[s][j] = sum_k A[s][k] B[k][j]  with
    //   A[s][k] = Y_s(pixel k)                  (constant over the walk: registers y_op)
    //   B[k][j] = aw of batch slot j at pixel k * grad_image_ch(pixel k)
    // The contraction index of MFMA step t, sub-index q (= lane >> 4) is pixel 16 q + t of the wave -- any bijection
    // serves a sum -- so that lane 16 q + j finds its sixteen B values (slot j, pixels 16 q .. 16 q + 15) and its
    // sixteen grad_image values contiguous in LDS:   y_op[t] = Y_{lane & 15}(pixel 16 q + t)   (rows s >= N_SH: 0)
    float y_op[16];
    int nb = 0;   // filled slots of the wave's open batch (wave-uniform)
    {
        float* tmp = s_B + wave * MB * BROW;   // [pixel][17]: 64 * 17 == MB * BROW floats of this wave
        static_assert(64 * 17 <= MB * BROW && MB * 48 <= MB * BROW, "scratch uses of the wave's B rows");
#pragma unroll
        for (int s2 = 0; s2 < 16; s2++) tmp[lane * 17 + s2] = s2 < N_SH ? Y[s2 < N_SH ? s2 : 0] : 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) s_gi[(wave * 3 + ch) * 64 + lane] = gi[ch];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int t = 0; t < 16; t++) y_op[t] = tmp[(16 * (lane >> 4) + t) * 17 + (lane & 15)];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // The GEMM of the open batch; its results are the wave's complete sums for (tile patch, splat): they go
    // straight to the global gradient rows (an LDS accumulator shared by the four waves needs 768 LDS float
    // atomics per batch, which cost more than the MFMAs: 0.15 of 0.69 ms at workload B)
    auto mma_flush = [&](int n_filled) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int j = lane & 15, q = lane >> 4;
        float* mine = s_B + wave * MB * BROW;
        const Vec4<float>* brow = reinterpret_cast<const Vec4<float>*>(mine + j * BROW + 16 * q);
        float b[16];
#pragma unroll
        for (int m4 = 0; m4 < 4; m4++) {
            const Vec4<float> v4 = brow[m4];
            b[4 * m4 + 0] = v4.x; b[4 * m4 + 1] = v4.y; b[4 * m4 + 2] = v4.z; b[4 * m4 + 3] = v4.w;
        }
        f32x4 acc[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const Vec4<float>* grow = reinterpret_cast<const Vec4<float>*>(s_gi + (wave * 3 + ch) * 64 + 16 * q);
            float g[16];
#pragma unroll
            for (int m4 = 0; m4 < 4; m4++) {
                const Vec4<float> v4 = grow[m4];
                g[4 * m4 + 0] = v4.x; g[4 * m4 + 1] = v4.y; g[4 * m4 + 2] = v4.z; g[4 * m4 + 3] = v4.w;
            }
            f32x4 even = {0, 0, 0, 0}, odd = {0, 0, 0, 0};   // two chains: the dependent-issue latency is 40 cycles
#pragma unroll
            for (int t = 0; t < 16; t += 2) {
                even = __builtin_amdgcn_mfma_f32_16x16x4f32(y_op[t], b[t] * g[t], even, 0, 0, 0);
                odd = __builtin_amdgcn_mfma_f32_16x16x4f32(y_op[t + 1], b[t + 1] * g[t + 1], odd, 0, 0, 0);
            }
            acc[ch] = even + odd;
        }
        // D: column j = lane & 15 (the batch slot), rows s = 4 q + r  ->  the wave's scratch as [slot][ch][16]
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();   // every lane has read its B values
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            Vec4<float> v4;
            v4.x = acc[ch][0]; v4.y = acc[ch][1]; v4.z = acc[ch][2]; v4.w = acc[ch][3];
            *reinterpret_cast<Vec4<float>*>(mine + j * 48 + ch * 16 + 4 * q) = v4;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // consecutive lanes, consecutive words of a gradient row
        for (int k = lane; k < n_filled * 48; k += 64) {
            const int row = k / 48, c = k - row * 48;
            const int ch = c >> 4, s2 = c & 15;
            if (s2 < N_SH) global_add(g_rgb + (size_t)s_bidx[wave * MB + row] * C + ch * N_SH + s2, mine[k]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    GS_STAT_DECL;
    GS_HALF_DECL;
    GS_STAT(0, 1);          // waves
    GS_STAT(7, n_tile);
    GS_STAT(8, n_used);
    // Q1 (render_backward.cu:185 compares a chunk-local index): k % REF_CH for k = base + i, i < RCHUNK <= REF_CH, is
    // base % REF_CH + i with at most one wrap -- one scalar division per CHUNK instead of a multiply-high sequence
    // (9 scalar instructions) per visit; exact mode never wraps
    static_assert(RCHUNK <= REF_CH, "one wrap per chunk");
    const int q1_wrap = exact ? 0x7fffffff : REF_CH;
    for (int chunk = (n_used - 1) / RCHUNK; chunk >= 0; chunk--) {
        const int base = chunk * RCHUNK;
        const int base_q = exact ? base : base % REF_CH;
        const int cnt = min(RCHUNK, n_used - base);
        GS_STAT(1, 1);
        __syncthreads();   // previous chunk fully flushed
        stage_chunk<float, N_SH, 1>(packed, rgb, sorted, s0 + base, cnt, tid, s_geom, s_col, s_idx, src_opacity, src_conic);
        GS_PHASE(0);
        if constexpr (RCHUNK == 64) {
            // one patch per wave: the records wave 0 staged have to be visible to the other three first
            __syncthreads();
            build_touch_masks_by_patch(s_geom, cnt, tid, tile % ntx, tile / ntx, s_mask);
        } else {
            // (no barrier in between: thread t tests the record thread t staged)
            build_touch_masks<float, RCHUNK>(s_geom, cnt, tid, tile % ntx, tile / ntx, s_mask);
        }
        __syncthreads();
        GS_PHASE(1);

        for (int word = (cnt - 1) >> 6; word >= 0; word--) {
          unsigned long long m = s_mask[wave][word];
          m = wave_uniform(m);
          unsigned long long hit = 0;   // the splats of this word whose slot the wave wrote
          while (m) {
            const int bit = 63 - __builtin_clzll(m);
            m &= ~(1ull << bit);
            const int i = (word << 6) + bit;
            const int k = base + i;
            int kq = base_q + i;   // = exact ? k : k % REF_CH
            kq = kq >= q1_wrap ? kq - q1_wrap : kq;
            const bool reach = k < nsp;   // render_backward.cu:131 (nsp == 0 outside the image)
            GS_STAT(2, 1);                          // visits
            if (ballot(reach) == 0) continue;      // wave-uniform: no lane reaches this splat
            GS_STAT(9, 1);                          // visits with a reaching lane
            GS_STAT(6, __popcll(ballot(reach)));
            GS_STAT_FLAG(st_in);
            // ---- the visit: k_render_bwd's (see there for the nine sums), with the record's colour replaced by the
            // pixel's and the three colour sums by the batch ----
            const float* rec = s_geom + i * GS_PACKED_WIDTH;
            const Vec4<float> g0 = *reinterpret_cast<const Vec4<float>*>(rec);       // u v r2 opacity
            const Vec4<float> g1 = *reinterpret_cast<const Vec4<float>*>(rec + 4);   // a b c det
            const Vec4<float> g2 = *reinterpret_cast<const Vec4<float>*>(rec + 8);   // 1/det (the colour words: unused)
            asm volatile("" ::"v"(g1.x), "v"(g1.y), "v"(g1.z), "v"(g1.w), "v"(g2.x), "v"(g2.y), "v"(g2.z), "v"(g2.w));
            const float du = pu - g0.x, dv = pv - g0.y;
            const float du2 = du * du, dv2 = dv * dv;
            // formed by the lanes that pass the alpha test only; `contrib` cuts the others out of the sums
            float aw = unset(), w = unset(), mh = unset(), duv = unset();
            bool contrib = false;
            if (reach && !(du2 + dv2 > g0.z)) {   // inside the cutoff radius
                GS_STAT_SET(st_in);
                // render_backward.cu:153-165 (multiplies by 1/det; the forward divides)
                duv = du * dv;
                mh = (g1.z * du * du - g1.w * du * dv + g1.x * dv * dv) * g2.x;   // g1.w = b + b (stage_chunk)
                // norm_prob = 0 unless mh > 0 (render_backward.cu:158-165) -- and then alpha = 0 fails the 1/255 test
                const float norm_prob = exp_neg_half(mh);
                float alpha = g0.w * norm_prob;
                if (alpha > Thr<float>::sat_gt()) alpha = Thr<float>::alpha_cap();   // min(0.9999, .)
                if ((mh > 0.0f) & (alpha >= Thr<float>::alpha_min())) {
                    contrib = true;
                    if (!bg_init) {   // render_backward.cu:172-181
                        const float bw = background_weight<float>(alpha, weight);
                        if (bw > Thr<float>::bgw_gt()) {
                            color_accum[0] += bg0 * bw;
                            color_accum[1] += bg1 * bw;
                            color_accum[2] += bg2 * bw;
                        }
                        bg_init = true;
                    }
                    // values only from here on (no threshold depends on them): contraction allowed
                    {
#pragma clang fp contract(fast)
                        const float r1ma = fast_rcp(1.0f - alpha);
                        if (kq < nsp - 1) weight = weight * r1ma;   // Q1 (chunk-local index) unless exact
                        aw = alpha * weight;
                        // grad_alpha (render_backward.cu:196-203), with the colour at this pixel's view direction
                        float col[3];
                        sh_to_rgb_contracted<float, N_SH>(s_col + i * CW, Y, col);
                        const float ga = (col[0] * weight - color_accum[0] * r1ma) * gi[0] +
                                         (col[1] * weight - color_accum[1] * r1ma) * gi[1] +
                                         (col[2] * weight - color_accum[2] * r1ma) * gi[2];
                        color_accum[0] += col[0] * aw;
                        color_accum[1] += col[1] * aw;
                        color_accum[2] += col[2] * aw;
                        w = norm_prob * ga;
                    }
                }
            }
            // a lane contributes iff it passed the alpha test; aw > 0 there (alpha >= 1/255, weight > 0)
            const float awz = contrib ? aw : 0.0f;
            const unsigned long long cmask = ballot(awz != 0.0f);
            GS_STAT(3, ballot(st_in) != 0);
            GS_STAT(4, cmask != 0);
            GS_STAT(5, __popcll(cmask));
            GS_HALF_VISIT(ballot(st_in));
            if (cmask == 0) continue;   // every reaching lane skipped the splat
            float val[9];
            const float wz = contrib ? w : 0.0f;
            const float awy = awz * Y[0];
            val[0] = awy * gi[0]; val[1] = awy * gi[1]; val[2] = awy * gi[2];   // (reduced, never flushed)
            val[3] = wz; val[4] = wz * du; val[5] = wz * dv;
            // (mh and duv of a lane that stayed outside are whatever an earlier visit left: 0 * x = 0 for every x)
            {
#pragma clang fp contract(fast)
                val[6] = mul_zero_wins((dv2 - g1.z * mh), wz);
                val[7] = mul_zero_wins((g1.y * mh - duv), wz);
                val[8] = mul_zero_wins((du2 - g1.x * mh), wz);
            }
            int slot_i = i * SV;   // (kept scalar: the compiler otherwise folds it into a 64-bit vector multiply-add)
            asm volatile("" : "+s"(slot_i));
            reduce9_to_slot(val, slot_stores, s_acc, slot_lane_base + slot_i);
            hit |= 1ull << bit;
            // column nb of the batch's B: this splat's aw at the wave's 64 pixels (0 where it does not contribute)
            s_B[(wave * MB + nb) * BROW + lane] = awz;
            if (lane == 0) s_bidx[wave * MB + nb] = s_idx[i];
            if (++nb == MB) {
                mma_flush(MB);
                nb = 0;
            }
          }
          if (lane == 0) s_hit[wave][word] = hit;
        }
        if (nb > 0) {
            mma_flush(nb);
            nb = 0;
        }
        GS_PHASE(2);
        GS_HALF_CHUNK(12);
        __syncthreads();
        GS_PHASE(3);
        // the flush: one global atomic per value per (splat, tile), the six geometric columns only (the colour
        // coefficients went out with the batches).  Phase 1: flush_sum_slots
        flush_sum_slots<RCHUNK, SV>(s_acc, s_geom, s_hit, tid, cnt);
        __syncthreads();
        // Phase 2, nine lanes = one row: seven rows per wave instruction, consecutive addresses (see k_render_bwd)
        const int sub = lane / SV, col = lane - sub * SV;   // lane 63: idle
        for (int r0 = wave * 7; r0 < cnt; r0 += 28) {
            const int r = r0 + sub;
            const bool in = lane < 63 && r < cnt && col >= 3;
            const float v = in ? s_acc[r * SV + col] : 0.0f;
            const unsigned long long nz = ballot(v != 0.0f);
            const bool any = in && ((nz >> (sub * SV)) & 0x1ffull) != 0;   // rows of zeros stay untouched
            GS_STAT(11, __popcll(ballot(any && col == 3)));   // flushed rows (col 3: the colour columns are not sent here)
            if (any) {
                const int g = s_idx[r];
                float* dst;
                if (col == 3) dst = g_opa + g;
                else if (col < 6) dst = g_uv + (size_t)g * 2 + (col - 4);
                else dst = g_conic + (size_t)g * 3 + (col - 6);
                global_add(dst, v);
            }
        }
        GS_PHASE(4);
    }
    GS_STAT_FLUSH(16);
}

// The fp64 reference kernel (gradcheck and the fp64 parity tests; never on a timed path): the same walk -- tile
// prologue, chunks from the tile's deepest used splat to the front, touch masks, Q1 -- with the plainest accumulation.
// One shared LDS row of 3 N_SH + 6 sums per staged splat, zero-filled per chunk; a visit sums each value over the wave
// (wave_sum) and lane 63 adds it to the row with an LDS atomic; the flush issues one global atomic per value per
// (splat, tile).  fp64 applies no cutoff radius and no alpha threshold (Thr<double>): every lane that reaches a
// splat contributes.  No slab, segments, depth cut, tile order or handed-over masks: launch_render_bwd is its only caller.
template <int N_SH>
__global__ __launch_bounds__(RB) void k_render_bwd_ref(
    const double* __restrict__ packed, const double* __restrict__ rgb, const double* __restrict__ view_dir,
    const int* __restrict__ ranges, const int* __restrict__ sorted, const double* __restrict__ bg,
    const int* __restrict__ nsp_in, const double* __restrict__ fw_in, const double* __restrict__ grad_image,
    int W, int H, int ntx, int tile0, int nt, double* __restrict__ g_rgb, double* __restrict__ g_opa,
    double* __restrict__ g_uv, double* __restrict__ g_conic, int exact, const double* __restrict__ src_opacity,
    const double* __restrict__ src_conic) {
    using T = double;
    constexpr int CW = ColW<N_SH>::value;
    constexpr int C = 3 * N_SH;
    constexpr int NV = C + 6;   // rgb coeffs, opacity, u, v, conic x3
    constexpr int REF_CH = ref_chunk<T>(N_SH);
    constexpr int RCHUNK = Chunk<T, N_SH>::value;
    constexpr int NWORD = RCHUNK / 64 > 0 ? RCHUNK / 64 : 1;
    __shared__ alignas(16) T s_geom[RCHUNK * GS_PACKED_WIDTH];
    __shared__ alignas(16) T s_col[N_SH > 1 ? RCHUNK * CW : 4];
    __shared__ int s_idx[RCHUNK];
    __shared__ T s_acc[RCHUNK * NV];   // [splat][NV]
    __shared__ int s_max[4];
    __shared__ unsigned long long s_mask[4][NWORD];

    const int t_local = tile_of_block(blockIdx.x, nt);
    if (t_local >= nt) return;
    const int tile = tile0 + t_local;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    const bool valid = px.u < W && px.v < H;
    const int s0 = ranges[tile];
    const int n_tile = ranges[tile + 1] - s0;
    if (n_tile <= 0) return;

    int nsp = 0;
    T weight = 0;
    T gi[3] = {0, 0, 0};
    T Y[N_SH];
    {
        T d[3] = {0, 0, 0};
        if (valid) {
            const size_t p = (size_t)px.v * W + px.u;
            nsp = nsp_in[p];
            weight = fw_in[p];
            gi[0] = grad_image[p * 3 + 0];
            gi[1] = grad_image[p * 3 + 1];
            gi[2] = grad_image[p * 3 + 2];
            if constexpr (N_SH > 1) {
                d[0] = view_dir[p * 3 + 0]; d[1] = view_dir[p * 3 + 1]; d[2] = view_dir[p * 3 + 2];
            }
        }
        if constexpr (N_SH > 1) sh_basis<T, N_SH>(d, Y);
        else Y[0] = T(GS_SH_0);
    }
    // the tile's deepest used splat (render_backward.cu:131 makes everything beyond it a no-op)
    int m = nsp;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, __shfl_xor(m, d));
    if (lane == 0) s_max[wave] = m;
    __syncthreads();
    const int n_used = min(n_tile, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
    if (n_used <= 0) return;

    const T pu = T(px.u), pv = T(px.v);
    T color_accum[3] = {0, 0, 0};
    bool bg_init = false;
    const T bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];

    // Q1 (render_backward.cu:185 compares a chunk-local index): k % REF_CH for k = base + i, i < RCHUNK <= REF_CH, is
    // base % REF_CH + i with at most one wrap; exact mode never wraps
    static_assert(RCHUNK <= REF_CH, "one wrap per chunk");
    const int q1_wrap = exact ? 0x7fffffff : REF_CH;
    for (int chunk = (n_used - 1) / RCHUNK; chunk >= 0; chunk--) {
        const int base = chunk * RCHUNK;
        const int base_q = exact ? base : base % REF_CH;
        const int cnt = min(RCHUNK, n_used - base);
        __syncthreads();   // previous chunk fully flushed
        stage_chunk<T, N_SH>(packed, rgb, sorted, s0 + base, cnt, tid, s_geom, s_col, s_idx, src_opacity, src_conic);
        for (int k = tid; k < cnt * NV; k += RB) s_acc[k] = 0;
        // (no barrier in between: thread t tests the record thread t staged)
        build_touch_masks<T, RCHUNK>(s_geom, cnt, tid, tile % ntx, tile / ntx, s_mask);
        __syncthreads();

        for (int word = (cnt - 1) >> 6; word >= 0; word--) {
          unsigned long long m = s_mask[wave][word];
          m = wave_uniform(m);
          while (m) {
            const int bit = 63 - __builtin_clzll(m);
            m &= ~(1ull << bit);
            const int i = (word << 6) + bit;
            const int k = base + i;
            int kq = base_q + i;   // = exact ? k : k % REF_CH
            kq = kq >= q1_wrap ? kq - q1_wrap : kq;
            const bool reach = k < nsp;   // render_backward.cu:131 (nsp == 0 outside the image)
            if (ballot(reach) == 0) continue;      // wave-uniform: no lane reaches this splat
            T val[NV];
#pragma unroll
            for (int j = 0; j < NV; j++) val[j] = 0;
            if (reach) {
                const T* rec = s_geom + i * GS_PACKED_WIDTH;
                const Vec4<T> g0 = *reinterpret_cast<const Vec4<T>*>(rec);       // u v r2 opacity
                const Vec4<T> g1 = *reinterpret_cast<const Vec4<T>*>(rec + 4);   // a b c det
                const T du = pu - g0.x, dv = pv - g0.y;
                const T a = g1.x, b = g1.y, c = g1.z, rdet = rec[8], opa = g0.w;
                // render_backward.cu:153-165 (multiplies by 1/det; forward divides)
                T norm_prob = 0;
                const T mh = (c * du * du - (b + b) * du * dv + a * dv * dv) * rdet;
                if (mh > T(0)) norm_prob = gexp<T>(T(-0.5) * mh);
                T alpha = opa * norm_prob;
                if (alpha > Thr<T>::sat_gt()) alpha = Thr<T>::alpha_cap();   // min(0.9999, .)
                if (!bg_init) {   // render_backward.cu:172-181
                    const T bw = background_weight<T>(alpha, weight);
                    if (bw > Thr<T>::bgw_gt()) {
                        color_accum[0] += bg0 * bw;
                        color_accum[1] += bg1 * bw;
                        color_accum[2] += bg2 * bw;
                    }
                    bg_init = true;
                }
                // From here on only gradient VALUES are formed (no threshold depends on
                // them): evaluated in T with the reference's formulas factored
                // (render_backward.cu:183-234) and contraction allowed; checked at 1e-4.
                {
#pragma clang fp contract(fast)
                    const T r1ma = fast_rcp(T(1) - alpha);
                    if (kq < nsp - 1) weight = weight * r1ma;   // Q1 (chunk-local index) unless exact
                    T col[3];
                    splat_colour<T, N_SH>(s_geom, s_col, i, Y, col);
                    const T aw = alpha * weight;
                    T grad_alpha = 0;
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        const T grl = aw * gi[ch];
#pragma unroll
                        for (int s = 0; s < N_SH; s++) val[N_SH * ch + s] = Y[s] * grl;
                        grad_alpha += (col[ch] * weight - color_accum[ch] * r1ma) * gi[ch];
                        color_accum[ch] += col[ch] * aw;
                    }
                    val[C + 0] = norm_prob * grad_alpha;
                    // d alpha / d mh^2 = -alpha_unclamped / 2; t = rdet * grad_mh
                    const T t = T(-0.5) * norm_prob * opa * grad_alpha * rdet;
                    const T A = c * du - b * dv;
                    const T B = a * dv - b * du;
                    val[C + 1] = T(-2) * A * t;           // :216-217
                    val[C + 2] = T(-2) * B * t;           // :218-219
                    val[C + 3] = (dv * dv - c * mh) * t;  // :221-229 with cf = mh^2 * rdet
                    val[C + 4] = (b * mh - du * dv) * t;
                    val[C + 5] = (du * du - a * mh) * t;
                }
            }
#pragma unroll
            for (int j = 0; j < NV; j++) val[j] = wave_sum(val[j]);   // total in lane 63
            if (lane == 63) {
#pragma unroll
                for (int j = 0; j < NV; j++)
                    __hip_atomic_fetch_add(&s_acc[i * NV + j], val[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
        }
        __syncthreads();
        // one global atomic per value per (splat, tile); rows of zeros stay untouched
        if (tid < cnt) {
            const int g = s_idx[tid];
            const T* a = s_acc + tid * NV;
            bool any = false;
#pragma unroll
            for (int j = 0; j < NV; j++) any |= (a[j] != T(0));
            if (any) {
#pragma unroll
                for (int j = 0; j < C; j++) global_add(g_rgb + (size_t)g * C + j, a[j]);
                global_add(g_opa + g, a[C + 0]);
                global_add(g_uv + (size_t)g * 2 + 0, a[C + 1]);
                global_add(g_uv + (size_t)g * 2 + 1, a[C + 2]);
                global_add(g_conic + (size_t)g * 3 + 0, a[C + 3]);
                global_add(g_conic + (size_t)g * 3 + 1, a[C + 4]);
                global_add(g_conic + (size_t)g * 3 + 2, a[C + 5]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// depth (depth.cu:7-115), fp32 only
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB) void k_render_depth(const float* __restrict__ packed,
                                                     const float* __restrict__ xyz_cam,
                                                     const int* __restrict__ ranges,
                                                     const int* __restrict__ sorted, int W, int H,
                                                     int ntx, int nt, float alpha_threshold,
                                                     float* __restrict__ depth) {
#ifndef GS_DEPTH_CHUNK
#define GS_DEPTH_CHUNK 256
#endif
    constexpr int RCHUNK = GS_DEPTH_CHUNK;
    __shared__ alignas(16) float s_geom[RCHUNK * GS_PACKED_WIDTH];
    __shared__ int s_idx[RCHUNK];
    const int tile = tile_of_block(blockIdx.x, nt);
    if (tile >= nt) return;
    const int tid = threadIdx.x;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    const bool valid = px.u < W && px.v < H;
    const int s0 = ranges[tile];
    const int n_tile = ranges[tile + 1] - s0;
    float acc = 0.0f;
    bool done = !valid;
    const float pu = (float)px.u, pv = (float)px.v;
    for (int base = 0; base < n_tile; base += RCHUNK) {
        const int cnt = min(RCHUNK, n_tile - base);
        if (tid < cnt) {
            const int g = sorted[s0 + base + tid];
            const Vec4<float>* src =
                reinterpret_cast<const Vec4<float>*>(packed + (size_t)g * GS_PACKED_WIDTH);
            Vec4<float>* dst = reinterpret_cast<Vec4<float>*>(s_geom + tid * GS_PACKED_WIDTH);
            dst[0] = src[0];
            dst[1] = src[1];
            s_idx[tid] = g;
        }
        __syncthreads();
        for (int i = 0; i < cnt; i++) {
            if (__ballot(!done) == 0) break;
            if (!done) {
                const Vec4<float> g0 =
                    *reinterpret_cast<const Vec4<float>*>(s_geom + i * GS_PACKED_WIDTH);       // u v r2 opa
                const Vec4<float> g1 =
                    *reinterpret_cast<const Vec4<float>*>(s_geom + i * GS_PACKED_WIDTH + 4);   // a b c det
                const float du = pu - g0.x, dv = pv - g0.y;
                const float a = g1.x, b = g1.y, c = g1.z, det = g1.w, opa = g0.w;
                const float mh = (c * du * du - (b + b) * du * dv + a * dv * dv) / det;
                float alpha = 0.0f;
                if (mh > 0.0f) alpha = opa * det_expf(-0.5f * mh);
                const float weight = alpha * (1.0 - acc);
                acc += weight;
                if (acc > alpha_threshold) {
                    const int g = s_idx[i];
                    const float x = xyz_cam[g * 3 + 0], y = xyz_cam[g * 3 + 1],
                                z = xyz_cam[g * 3 + 2];
                    depth[(size_t)px.v * W + px.u] = __builtin_sqrtf(x * x + y * y + z * z);
                    done = true;
                }
            }
        }
        if (__syncthreads_and(done)) break;
    }
}

// ---------------------------------------------------------------------------------------------------
// differentiable depth and accumulated opacity (no reference counterpart), fp32, one colour coefficient
// ---------------------------------------------------------------------------------------------------
// For pixel p and the entries k < num_splats_per_pixel[p] the colour forward walked, with alpha_k and the
// contribute decision formed by render_tile_fwd_fused's own expressions (zalpha_alpha below):
//   T_k = prod_{j < k, contributing} (1 - alpha_j)      w_k = alpha_k T_k
//   depth[p] = sum w_k z_k  (z = xyz_camera_frame[:, 2])      alpha[p] = sum w_k      T_end = the product over all
// No background, no normalisation.  The kernels stand BESIDE the colour kernels (whose ISA is left alone): plain walks
// of the touch masks, one record read per visit, no flags, costs, segments or handed-over masks.  They read
// num_splats_per_pixel and never look beyond it, so they need no saturation test and are correct on prefix-sorted
// lists (a tile is ordered as far as any of its pixels walked).
// The walks are render_map_fwd and render_map_bwd below, shared with the feature maps further down: everything about
// alpha, T, the order of the sums and the slab is there, once; z enters through the depth policies (DepthFwd, DepthBwd).
//
// alpha of one (pixel, staged record) pair and whether it contributes -- the forward's decisions, bit for bit: the
// cutoff radius, the IEEE quotient from the stored reciprocal, exp_neg_half, zero unless mh > 0, alpha >= 1/255.
struct ZalphaVisit {
    float du, dv, mh, norm_prob, alpha;
    bool contrib;
};
__device__ __forceinline__ ZalphaVisit zalpha_alpha(const Vec4<float>& g0, const Vec4<float>& g1, float rdet, float pu,
                                                    float pv, bool reach) {
    ZalphaVisit o;
    o.du = pu - g0.x;
    o.dv = pv - g0.y;
    o.mh = 0.0f; o.norm_prob = 0.0f; o.alpha = 0.0f;
    o.contrib = false;
    if (reach && !(o.du * o.du + o.dv * o.dv > g0.z)) {
        const float tb = g1.y + g1.y;
        o.mh = div_by_reciprocal(g1.z * o.du * o.du - tb * o.du * o.dv + g1.x * o.dv * o.dv, g1.w, rdet);
        o.norm_prob = exp_neg_half(o.mh);
        o.alpha = g0.w * o.norm_prob;
        o.contrib = (o.mh > 0.0f) & !(o.alpha < Thr<float>::alpha_min());
    }
    return o;
}

// the deepest entry any pixel of the workgroup / of this wave walked (0 outside the image); barrier inside
__device__ __forceinline__ void zalpha_reach(int nsp, int n_tile, int tid, int* s_max, int& n_used, int& wave_used) {
    int m = nsp;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = max(m, __shfl_xor(m, d));
    if ((tid & 63) == 0) s_max[tid >> 6] = m;
    __syncthreads();
    n_used = min(n_tile, max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])));
    wave_used = __builtin_amdgcn_readfirstlane(m);
}

constexpr int MAP_FWD_CHUNK = 256;   // entries staged per chunk of the forward walk
constexpr int MAP_BWD_CHUNK = 64;    // of the backward walk: one mask word, one slot of nine sums per (wave, entry)

// The forward walk of one tile (one workgroup, a wave per 8 x 8 patch): alpha and T_end [H, W] of the tile's pixels
// inside the image, and the channel policy's map.  T_end is stored itself: at alpha = 0.99999 the difference
// 1 - alpha formed in fp32 is good to about 1 %.  The pixel's N channel sums M are locals of the walk, beside T and A
// (as members of the policy object they cost k_render_features_fwd<4> about 0.6 %).  Ch supplies
//   N                                               the number of channel sums per pixel
//   stage(sorted, first, cnt, tid, s_geom, s_idx)   the chunk's channel values into LDS, beside the records (s_idx: the
//                                                   Gaussian indices stage_chunk kept, nullptr in the forward)
//   add(M, w, rec, i, T)                            staged entry i (rec: its record) enters the sums with weight w;
//                                                   T: the transmittance in front of it (only MedianFwd reads it)
//   store(M, p)                                     the sums to the map
template <class Ch>
__device__ __forceinline__ void render_map_fwd(
    const Ch ch, const float* __restrict__ packed, const int* __restrict__ ranges, const int* __restrict__ sorted,
    const int* __restrict__ nsp_in, int W, int H, int ntx, int tile0, int nt, float* __restrict__ alpha_out,
    float* __restrict__ t_out, float* s_geom, unsigned long long (*s_mask)[MAP_FWD_CHUNK / 64], int* s_max) {
    constexpr int RCHUNK = MAP_FWD_CHUNK;
    constexpr int NW = RCHUNK / 64;
    const int t_local = tile_of_block(blockIdx.x, nt);
    if (t_local >= nt) return;
    const int tile = tile0 + t_local;
    const int tid = threadIdx.x, wave = tid >> 6;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    const bool valid = px.u < W && px.v < H;
    const size_t p = (size_t)px.v * W + px.u;
    const int s0 = ranges[tile];
    const int n_tile = ranges[tile + 1] - s0;
    const int nsp = valid ? nsp_in[p] : 0;
    int n_used, wave_used;
    zalpha_reach(nsp, n_tile, tid, s_max, n_used, wave_used);
    const float pu = float(px.u), pv = float(px.v);
    float T = 1.0f, A = 0.0f;
    float M[Ch::N];   // the pixel's sums of the map's channels
#pragma unroll
    for (int c = 0; c < Ch::N; c++) M[c] = 0.0f;
    for (int base = 0; base < n_used; base += RCHUNK) {
        const int cnt = min(RCHUNK, n_used - base);
        if (base > 0) __syncthreads();   // the previous chunk's readers are done
        stage_chunk<float, 1>(packed, nullptr, sorted, s0 + base, cnt, tid, s_geom, nullptr, nullptr);
        ch.stage(sorted, s0 + base, cnt, tid, s_geom, nullptr);
        // (no barrier in between: thread t tests the record thread t staged)
        build_touch_masks<float, RCHUNK>(s_geom, cnt, tid, tile % ntx, tile / ntx, s_mask);
        __syncthreads();
        for (int word = 0; word < NW && word * 64 < cnt; word++) {
            if (base + word * 64 >= wave_used) break;   // wave-uniform: no pixel of the patch walked this far
            unsigned long long m = wave_uniform(s_mask[wave][word]);
            while (m) {
                const int i = word * 64 + __builtin_ctzll(m);
                m &= m - 1;
                const int k = base + i;
                if (k >= wave_used) break;
                const float* rec = s_geom + i * GS_PACKED_WIDTH;
                const Vec4<float> g0 = *reinterpret_cast<const Vec4<float>*>(rec);       // u v r2 opacity
                const Vec4<float> g1 = *reinterpret_cast<const Vec4<float>*>(rec + 4);   // a b c det
                const ZalphaVisit v = zalpha_alpha(g0, g1, rec[8], pu, pv, k < nsp);
                if (v.contrib) {
                    const float w = v.alpha * T;
                    ch.add(M, w, rec, i, T);
                    A += w;
                    T = __builtin_fmaf(-v.alpha, T, T);   // T (1 - alpha), one rounding
                }
            }
        }
    }
    if (valid) {
        ch.store(M, p);
        alpha_out[p] = A;
        t_out[p] = T;
    }
}

// The true derivative of a map and of alpha (the contribute / stop decisions held constant), back to front from T_end
// with c_k = g_alpha + <g_map, channels of entry k>:
//   T_k = T / (1 - alpha_k)      dL/dalpha_k = T_k c_k - S / (1 - alpha_k)      S += alpha_k T_k c_k
// and alpha -> opacity, u, v, conic as k_render_bwd chains them (the per-splat factor -0.5 opacity / det in
// flush_sum_slots).  No walk quirk is replicated: this output has no reference to be compatible with.
// alpha above 0.9999 enters the derivative as 0.9999, as in k_render_bwd (Q4).  Nine sums per (wave, entry) -- the
// policy's column 0, two zeros | opacity | w du, w dv | conic 3 -- through reduce9_to_slot into the wave's own LDS
// slot, the four waves' slots added per chunk (flush_sum_slots), then nine lanes per row, one global atomic per value
// per (entry, tile): columns 3..8 of the [V, 9] slab, columns 0..2 wherever the policy sends them (the slab's colour
// columns are not touched); rows of zeros stay untouched.  Chunks of 64 entries, from the tile's deepest
// num_splats_per_pixel to the front, tiles in grid order.  Ch supplies
//   stage(sorted, first, cnt, tid, s_geom, s_idx)   as the forward's
//   load(p)                                         the pixel's incoming map gradient (pixels outside the image: zeros)
//   begin(lane, wave)                               once the tile is known to have work
//   c(ga, g2, i, alpha, T, r1ma)                    c_k of staged entry i (g2: words 8..11 of its record).  alpha: the
//                                                   capped alpha_k, T: the transmittance BEHIND the entry, r1ma:
//                                                   1 / (1 - alpha_k) -- a policy whose c_k depends on w_k forms it as
//                                                   alpha * (T * r1ma), the expression of the walk's own w_k, which
//                                                   is formed after the call (moving the call below it reorders
//                                                   every instantiation; profiles/r17/map_bwd_isa.txt)
//   column0(aT)                                     the contributing lane's input to sum 0, from w_k = alpha_k T_k;
//                                                   called after c() of the same entry
//   visited(aT, g)                                  after the slot of an entry (Gaussian g) is written; aT = 0 in lanes
//                                                   that did not contribute
//   send(g, col, x)                                 the sum x of column col < 3 of Gaussian g's row, to where it belongs
//   finish()                                        after the last chunk
template <class Ch>
__device__ __forceinline__ void render_map_bwd(
    Ch& ch, const float* __restrict__ packed, const int* __restrict__ ranges, const int* __restrict__ sorted,
    const int* __restrict__ nsp_in, const float* __restrict__ t_in, const float* __restrict__ g_alpha, int W, int H,
    int ntx, int tile0, int nt, float* __restrict__ slab, float* s_geom, int* s_idx, float* s_acc, int* s_max,
    unsigned long long (*s_mask)[1], unsigned long long (*s_hit)[1]) {
    constexpr int SV = 9;
    constexpr int RCHUNK = MAP_BWD_CHUNK;
    const int t_local = tile_of_block(blockIdx.x, nt);
    if (t_local >= nt) return;
    const int tile = tile0 + t_local;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    const bool valid = px.u < W && px.v < H;
    const int s0 = ranges[tile];
    const int n_tile = ranges[tile + 1] - s0;
    if (n_tile <= 0) return;
    int nsp = 0;
    float T = 1.0f, ga = 0.0f;
    if (valid) {
        const size_t p = (size_t)px.v * W + px.u;
        nsp = nsp_in[p];
        T = t_in[p];
        ch.load(p);
        if (g_alpha != nullptr) ga = g_alpha[p];
    }
    int n_used, wave_used;
    zalpha_reach(nsp, n_tile, tid, s_max, n_used, wave_used);
    if (n_used <= 0) return;
    const float pu = float(px.u), pv = float(px.v);
    const int slot_off = slot_lane_offset(lane);
    const bool slot_stores = slot_off >= 0;
    const int slot_lane_base = wave * RCHUNK * SV + (slot_stores ? slot_off : 0);
    ch.begin(lane, wave);
    float S = 0.0f;   // sum of alpha_j T_j c_j over the contributors behind the current entry
    for (int chunk = (n_used - 1) / RCHUNK; chunk >= 0; chunk--) {
        const int base = chunk * RCHUNK;
        const int cnt = min(RCHUNK, n_used - base);
        __syncthreads();   // previous chunk fully flushed
        stage_chunk<float, 1>(packed, nullptr, sorted, s0 + base, cnt, tid, s_geom, nullptr, s_idx);
        ch.stage(sorted, s0 + base, cnt, tid, s_geom, s_idx);
        // (no barrier in between: thread t tests the record thread t staged)
        build_touch_masks<float, RCHUNK>(s_geom, cnt, tid, tile % ntx, tile / ntx, s_mask);
        __syncthreads();
        unsigned long long m = wave_uniform(s_mask[wave][0]);
        unsigned long long hit = 0;   // the entries of this chunk whose slot the wave wrote
        while (m) {
            const int i = 63 - __builtin_clzll(m);
            m &= ~(1ull << i);
            const int k = base + i;
            if (k >= wave_used) continue;   // wave-uniform: no pixel of the patch walked this far
            const float* rec = s_geom + i * GS_PACKED_WIDTH;
            const Vec4<float> g0 = *reinterpret_cast<const Vec4<float>*>(rec);       // u v r2 opacity
            const Vec4<float> g1 = *reinterpret_cast<const Vec4<float>*>(rec + 4);   // a b c det
            const Vec4<float> g2 = *reinterpret_cast<const Vec4<float>*>(rec + 8);   // 1/det, z (depth)
            const ZalphaVisit v = zalpha_alpha(g0, g1, g2.x, pu, pv, k < nsp);
            if (ballot(v.contrib) == 0) continue;   // every reaching lane skipped the entry
            float v0 = 0.0f, w = 0.0f, aT = 0.0f;
            if (v.contrib) {
                float alpha = v.alpha;
                if (alpha > Thr<float>::sat_gt()) alpha = Thr<float>::alpha_cap();   // min(0.9999, .)
                const float r1ma = fast_rcp(1.0f - alpha);
                const float c = ch.c(ga, g2, i, alpha, T, r1ma);
                T = T * r1ma;                        // T_k: the transmittance in front of the entry
                aT = alpha * T;                      // w_k
                const float dalpha = T * c - S * r1ma;
                S = __builtin_fmaf(aT, c, S);
                v0 = ch.column0(aT);
                w = v.norm_prob * dalpha;
            }
            float val[9];
            const float du2 = v.du * v.du, dv2 = v.dv * v.dv, duv = v.du * v.dv;
            val[0] = v0; val[1] = 0.0f; val[2] = 0.0f;
            val[3] = w; val[4] = w * v.du; val[5] = w * v.dv;
            val[6] = (dv2 - g1.z * v.mh) * w;
            val[7] = (g1.y * v.mh - duv) * w;
            val[8] = (du2 - g1.x * v.mh) * w;
            int slot_i = i * SV;
            asm volatile("" : "+s"(slot_i));
            reduce9_to_slot(val, slot_stores, s_acc, slot_lane_base + slot_i);
            hit |= 1ull << i;
            ch.visited(aT, s_idx[i]);
        }
        if (lane == 0) s_hit[wave][0] = hit;
        __syncthreads();
        // (the thread index of the flush is formed here, inside the chunk loop, as slot_i above: left to the compiler, the
        // twelve slot addresses of flush_sum_slots are hoisted over the whole walk and k_render_features_bwd<4> takes 120
        // VGPRs where its own body took 104; profiles/r12/map_walk_isa.txt)
        int row_tid = tid;
        asm volatile("" : "+v"(row_tid));
        flush_sum_slots<RCHUNK, SV>(s_acc, s_geom, s_hit, row_tid, cnt);
        __syncthreads();
        // nine lanes = one row (seven rows per wave instruction, see k_render_bwd)
        const int sub = lane / SV, col = lane - sub * SV;   // lane 63: idle
        for (int r0 = wave * 7; r0 < cnt; r0 += 28) {
            const int r = r0 + sub;
            const bool in = lane < 63 && r < cnt;
            const float x = in ? s_acc[r * SV + col] : 0.0f;
            const unsigned long long nz = ballot(x != 0.0f);
            const bool any = in && ((nz >> (sub * SV)) & 0x1ffull) != 0;
            if (any) {
                const int g = s_idx[r];
                if (col >= 3) global_add(slab + (size_t)g * SV + col, x);
                else ch.send(g, col, x);
            }
        }
    }
    ch.finish();
}

// The depth policy: one channel, z = xyz_camera_frame[:, 2], staged into the record's first colour word (word 9, which
// nobody here reads as a colour).
struct DepthChannel {
    const float* __restrict__ xyz_cam;
    __device__ __forceinline__ void stage(const int* __restrict__ sorted, int first, int cnt, int tid, float* s_geom,
                                          const int* s_idx) const {
        if (tid < cnt) {
            const int g = s_idx != nullptr ? s_idx[tid] : sorted[first + tid];   // (what this thread staged)
            s_geom[tid * GS_PACKED_WIDTH + 9] = xyz_cam[(size_t)g * 3 + 2];
        }
    }
};
struct DepthFwd : DepthChannel {
    float* __restrict__ depth;
    static constexpr int N = 1;
    __device__ __forceinline__ void add(float (&D)[1], float w, const float* rec, int, float) const {
        D[0] = __builtin_fmaf(w, rec[9], D[0]);
    }
    __device__ __forceinline__ void store(const float (&D)[1], size_t p) const { depth[p] = D[0]; }
};
// c_k = g_depth z_k + g_alpha, dL/dz_k = g_depth w_k: sum 0 of the slot, added to grad_z[g]
struct DepthBwd : DepthChannel {
    const float* __restrict__ g_depth;
    float* __restrict__ grad_z;
    float gd = 0.0f;
    __device__ __forceinline__ void load(size_t p) {
        if (g_depth != nullptr) gd = g_depth[p];
    }
    __device__ __forceinline__ void begin(int, int) const {}
    __device__ __forceinline__ float c(float ga, const Vec4<float>& g2, int, float, float, float) const {
        return __builtin_fmaf(gd, g2.y, ga);
    }
    __device__ __forceinline__ float column0(float aT) const { return gd * aT; }
    __device__ __forceinline__ void visited(float, int) const {}
    __device__ __forceinline__ void send(int g, int col, float x) const {
        if (col == 0) global_add(grad_z + g, x);
    }
    __device__ __forceinline__ void finish() const {}
};

__global__ __launch_bounds__(RB) void k_render_zalpha_fwd(
    const float* __restrict__ packed, const float* __restrict__ xyz_cam, const int* __restrict__ ranges,
    const int* __restrict__ sorted, const int* __restrict__ nsp_in, int W, int H, int ntx, int tile0, int nt,
    float* __restrict__ depth, float* __restrict__ alpha_out, float* __restrict__ t_out) {
    __shared__ alignas(16) float s_geom[MAP_FWD_CHUNK * GS_PACKED_WIDTH];
    __shared__ unsigned long long s_mask[4][MAP_FWD_CHUNK / 64];
    __shared__ int s_max[4];
    DepthFwd ch{{xyz_cam}, depth};
    render_map_fwd(ch, packed, ranges, sorted, nsp_in, W, H, ntx, tile0, nt, alpha_out, t_out, s_geom, s_mask, s_max);
}

__global__ __launch_bounds__(RB) void k_render_zalpha_bwd(
    const float* __restrict__ packed, const float* __restrict__ xyz_cam, const int* __restrict__ ranges,
    const int* __restrict__ sorted, const int* __restrict__ nsp_in, const float* __restrict__ t_in,
    const float* __restrict__ g_depth, const float* __restrict__ g_alpha, int W, int H, int ntx, int tile0, int nt,
    float* __restrict__ slab, float* __restrict__ grad_z) {
    __shared__ alignas(16) float s_geom[MAP_BWD_CHUNK * GS_PACKED_WIDTH];
    __shared__ int s_idx[MAP_BWD_CHUNK];
    __shared__ float s_acc[4 * MAP_BWD_CHUNK * 9];   // [wave][entry][9]
    __shared__ int s_max[4];
    __shared__ unsigned long long s_mask[4][1];
    __shared__ unsigned long long s_hit[4][1];       // slots written by each wave
    DepthBwd ch{{xyz_cam}, g_depth, grad_z};
    render_map_bwd(ch, packed, ranges, sorted, nsp_in, t_in, g_alpha, W, H, ntx, tile0, nt, slab, s_geom, s_idx, s_acc,
                   s_max, s_mask, s_hit);
}

// ---------------------------------------------------------------------------------------------------
// depth distortion (no reference counterpart), fp32: the weight a pixel spreads over depth
// ---------------------------------------------------------------------------------------------------
// With alpha_k, the contribute decision, T_k and w_k of the depth kernels above (the same walk: depth, alpha and T_end
// come out with k_render_zalpha_fwd's bits), A_<k = sum_{j<k} w_j and D_<k = sum_{j<k} w_j z_j over the contributors in
// front of k:
//   distortion[p] = 2 sum_k w_k (z_k A_<k - D_<k) = sum_{i != j} w_i w_j (z_later - z_earlier)
// in LIST order, no |.|: on lists sorted by z (the frame's own) that is sum_{i,j} w_i w_j |z_i - z_j|, the distortion
// loss of Mip-NeRF 360 without its normalisations.  The forward is render_map_fwd with three sums -- D, X and the
// policy's own copy of A (the walk's A is not handed to add(); the copy sees the same additions, the same bits):
//   X = fma(w, fma(z, A, -D), X)      D = fma(w, z, D)      A += w            the store is 2 X
struct DistortionFwd : DepthChannel {
    float* __restrict__ depth;
    float* __restrict__ distortion;
    static constexpr int N = 3;   // D | X | A
    __device__ __forceinline__ void add(float (&M)[3], float w, const float* rec, int, float) const {
        const float z = rec[9];
        M[1] = __builtin_fmaf(w, __builtin_fmaf(z, M[2], -M[0]), M[1]);
        M[0] = __builtin_fmaf(w, z, M[0]);
        M[2] += w;
    }
    __device__ __forceinline__ void store(const float (&M)[3], size_t p) const {
        depth[p] = M[0];
        distortion[p] = 2.0f * M[1];
    }
};

__global__ __launch_bounds__(RB) void k_render_distortion_fwd(
    const float* __restrict__ packed, const float* __restrict__ xyz_cam, const int* __restrict__ ranges,
    const int* __restrict__ sorted, const int* __restrict__ nsp_in, int W, int H, int ntx, int tile0, int nt,
    float* __restrict__ distortion, float* __restrict__ depth, float* __restrict__ alpha_out,
    float* __restrict__ t_out) {
    __shared__ alignas(16) float s_geom[MAP_FWD_CHUNK * GS_PACKED_WIDTH];
    __shared__ unsigned long long s_mask[4][MAP_FWD_CHUNK / 64];
    __shared__ int s_max[4];
    DistortionFwd ch{{xyz_cam}, depth, distortion};
    render_map_fwd(ch, packed, ranges, sorted, nsp_in, W, H, ntx, tile0, nt, alpha_out, t_out, s_geom, s_mask, s_max);
}

// The true derivative of distortion, depth and alpha together (decisions held constant, alpha above 0.9999 as 0.9999,
// no walk quirk): a policy of render_map_bwd like DepthBwd.  c_k of the distortion needs w_k, which the walk forms after
// it has called c(); the hook's arguments alpha, T and 1 / (1 - alpha) let the policy form it with the walk's own
// expression (one value in the ISA).  The suffix sums A_>k = sum_{j>k} w_j and D_>k = sum_{j>k} w_j z_j are carried, the
// prefixes come from the forward's totals alpha[p] and depth[p]:
//   A_<k = alpha[p] - A_>k - w_k      D_<k = depth[p] - D_>k - w_k z_k
//   e_k = 2 [z_k (A_<k - A_>k) - D_<k + D_>k]                        (d distortion / d w_k)
//   c_k = fma(g_dist, e_k, fma(g_depth, z_k, g_alpha))               (g_dist = 0: the depth kernel's c_k, bit for bit)
//   dL/dz_k = g_depth w_k + g_dist 2 w_k (A_<k - A_>k)               (sum 0 of the slot, to grad_z)
// then dL/dalpha_k = T_k c_k - S / (1 - alpha_k), S = fma(w_k, c_k, S) and the chain to opacity, u, v, conic, the nine
// sums, the slots and the flush are the walk's.
struct DistortionBwd : DepthChannel {
    const float* __restrict__ depth_in;
    const float* __restrict__ alpha_in;
    const float* __restrict__ g_dist;
    const float* __restrict__ g_depth;
    float* __restrict__ grad_z;
    float gx = 0.0f, gd = 0.0f;
    float A_tot = 0.0f, D_tot = 0.0f;   // the forward's totals of the pixel
    float A_gt = 0.0f, D_gt = 0.0f;     // sums of w_j and of w_j z_j over the contributors behind the current entry
    float dA = 0.0f;                    // A_<k - A_>k of the entry, from c() to column0()
    __device__ __forceinline__ void load(size_t p) {
        // (the gradients first, the totals last: with the totals first the kernel measured 1.5 % slower at workload D,
        // the instructions of the visit loop being the same; profiles/r17/README.md)
        if (g_dist != nullptr) gx = g_dist[p];
        if (g_depth != nullptr) gd = g_depth[p];
        A_tot = alpha_in[p];
        D_tot = depth_in[p];
    }
    __device__ __forceinline__ void begin(int, int) const {}
    __device__ __forceinline__ float c(float ga, const Vec4<float>& g2, int, float alpha, float T, float r1ma) {
        const float z = g2.y;
        const float aT = alpha * (T * r1ma);   // w_k, the walk's expression
        const float wz = aT * z;
        const float A_lt = A_tot - A_gt - aT;
        const float D_lt = D_tot - D_gt - wz;
        dA = A_lt - A_gt;
        const float e = 2.0f * (z * dA - D_lt + D_gt);
        A_gt += aT;
        D_gt += wz;
        return __builtin_fmaf(gx, e, __builtin_fmaf(gd, z, ga));
    }
    __device__ __forceinline__ float column0(float aT) const { return __builtin_fmaf(gx, 2.0f * aT * dA, gd * aT); }
    __device__ __forceinline__ void visited(float, int) const {}
    __device__ __forceinline__ void send(int g, int col, float x) const {
        if (col == 0) global_add(grad_z + g, x);
    }
    __device__ __forceinline__ void finish() const {}
};

__global__ __launch_bounds__(RB) void k_render_distortion_bwd(
    const float* __restrict__ packed, const float* __restrict__ xyz_cam, const int* __restrict__ ranges,
    const int* __restrict__ sorted, const int* __restrict__ nsp_in, const float* __restrict__ t_in,
    const float* __restrict__ depth_in, const float* __restrict__ alpha_in, const float* __restrict__ g_dist,
    const float* __restrict__ g_depth, const float* __restrict__ g_alpha, int W, int H, int ntx, int tile0, int nt,
    float* __restrict__ slab, float* __restrict__ grad_z) {
    __shared__ alignas(16) float s_geom[MAP_BWD_CHUNK * GS_PACKED_WIDTH];
    __shared__ int s_idx[MAP_BWD_CHUNK];
    __shared__ float s_acc[4 * MAP_BWD_CHUNK * 9];   // [wave][entry][9]
    __shared__ int s_max[4];
    __shared__ unsigned long long s_mask[4][1];
    __shared__ unsigned long long s_hit[4][1];       // slots written by each wave
    DistortionBwd ch{{xyz_cam}, depth_in, alpha_in, g_dist, g_depth, grad_z};
    render_map_bwd(ch, packed, ranges, sorted, nsp_in, t_in, g_alpha, W, H, ntx, tile0, nt, slab, s_geom, s_idx, s_acc,
                   s_max, s_mask, s_hit);
}

// ---------------------------------------------------------------------------------------------------
// median depth (2DGS's depth_ratio = 1), fp32: the z of the entry at which T falls through 0.5
// ---------------------------------------------------------------------------------------------------
// With alpha_k, the contribute decision and T_k (the transmittance in front of entry k) of the depth kernels above (the
// same walk: depth, alpha and T_end come out with k_render_zalpha_fwd's bits), the MEDIAN ENTRY of a pixel is its last
// contributing entry with T_k > 0.5f -- the entry during which T falls to 0.5 or below, or the last contributor if it
// never does (2DGS: `if (T > 0.5) median = depth`, evaluated before the blend).
//   median_depth[p] = z of that entry's Gaussian, not weighted, not normalised (0 without a contributor)
//   median_index[p] = that Gaussian's sorted_gaussians value (-1 without a contributor)
// The forward is render_map_fwd with three walk locals: D as DepthFwd's, the median z, and the BITS of the median
// Gaussian's index + 1 (0, the locals' initial value, is "none": the store subtracts the 1).  The index of a staged
// entry is not in LDS in the forward (s_idx is nullptr there), so stage() puts it, + 1, beside z: word 10 of the
// record, the second colour word, which like word 9 nobody here reads as a colour.  The pair is only ever copied (LDS
// -> register -> select -> store): no float instruction sees the index bits.
struct MedianFwd : DepthChannel {
    float* __restrict__ depth;
    float* __restrict__ median_depth;
    int* __restrict__ median_index;
    static constexpr int N = 3;   // D | z of the median entry | bits of (its Gaussian + 1)
    __device__ __forceinline__ void stage(const int* __restrict__ sorted, int first, int cnt, int tid, float* s_geom,
                                          const int* s_idx) const {
        if (tid < cnt) {
            const int g = s_idx != nullptr ? s_idx[tid] : sorted[first + tid];   // (what this thread staged)
            s_geom[tid * GS_PACKED_WIDTH + 9] = xyz_cam[(size_t)g * 3 + 2];
            s_geom[tid * GS_PACKED_WIDTH + 10] = __int_as_float(g + 1);
        }
    }
    __device__ __forceinline__ void add(float (&M)[3], float w, const float* rec, int, float T) const {
        const float z = rec[9];
        M[0] = __builtin_fmaf(w, z, M[0]);
        if (T > 0.5f) {   // T in front of the entry: every contributor up to the crossing overwrites the pair
            M[1] = z;
            M[2] = rec[10];
        }
    }
    __device__ __forceinline__ void store(const float (&M)[3], size_t p) const {
        depth[p] = M[0];
        median_depth[p] = M[1];
        median_index[p] = __float_as_int(M[2]) - 1;
    }
};

__global__ __launch_bounds__(RB) void k_render_median_fwd(
    const float* __restrict__ packed, const float* __restrict__ xyz_cam, const int* __restrict__ ranges,
    const int* __restrict__ sorted, const int* __restrict__ nsp_in, int W, int H, int ntx, int tile0, int nt,
    float* __restrict__ median_depth, int* __restrict__ median_index, float* __restrict__ depth,
    float* __restrict__ alpha_out, float* __restrict__ t_out) {
    __shared__ alignas(16) float s_geom[MAP_FWD_CHUNK * GS_PACKED_WIDTH];
    __shared__ unsigned long long s_mask[4][MAP_FWD_CHUNK / 64];
    __shared__ int s_max[4];
    MedianFwd ch{{xyz_cam}, depth, median_depth, median_index};
    render_map_fwd(ch, packed, ranges, sorted, nsp_in, W, H, ntx, tile0, nt, alpha_out, t_out, s_geom, s_mask, s_max);
}

// dL/dz of the median depth, the choice of entry held constant: grad_z[median_index[p]] += grad_median_depth[p].  No
// list walk: a scatter, one workgroup per tile with the walks' pixel mapping (a wave = an 8 x 8 patch, whose pixels
// mostly share a few Gaussians).  The wave loops over the distinct indices it holds -- the first pending lane's index,
// the ballot of its matches, their sum -- and one lane issues ONE atomic per (wave, distinct Gaussian): a lane-per-pixel
// atomic onto one large foreground Gaussian is the one-row contention that runs an order of magnitude slower.
// Pixels outside the image and pixels without a contributor (-1) add nothing.
__global__ __launch_bounds__(RB) void k_median_depth_bwd(const int* __restrict__ median_index,
                                                         const float* __restrict__ g_median, int W, int H, int ntx,
                                                         int tile0, int nt, float* __restrict__ grad_z) {
    const int t_local = tile_of_block(blockIdx.x, nt);
    if (t_local >= nt) return;
    const int tile = tile0 + t_local;
    const int tid = threadIdx.x, lane = tid & 63;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    int g = -1;
    float x = 0.0f;
    if (px.u < W && px.v < H) {
        const size_t p = (size_t)px.v * W + px.u;
        g = median_index[p];
        if (g >= 0) x = g_median[p];
    }
    unsigned long long todo = ballot(g >= 0);
    while (todo) {   // wave-uniform
        const int leader = __builtin_ctzll(todo);
        const int gl = __builtin_amdgcn_readlane(g, leader);
        const bool mine = g == gl;
        float s = mine ? x : 0.0f;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
        if (lane == leader) global_add(grad_z + gl, s);
        todo &= ~ballot(mine);
    }
}

// ---------------------------------------------------------------------------------------------------
// per-Gaussian feature vectors composited with the frame's weights (no reference counterpart), fp32
// ---------------------------------------------------------------------------------------------------
// render_map_fwd / render_map_bwd with C <= 32 caller-supplied channels in place of the one channel z:
//   feature_map[p, c] = sum w_k features[g_k, c]      alpha[p] = sum w_k      T_end
// The walk is the depth kernels' own, so alpha and T_end are bit-equal to k_render_zalpha_fwd's and a channel holding
// z gives its depth.  The policies are templated on a padded channel count CP and instantiated for CP = 4, 8, 16, 32
// (the next one at or above n_channels runs): a feature row is staged into LDS beside the geometry records with a
// pitch of CP floats (16-byte aligned, read as ds_read_b128 broadcasts), the channels from n_channels to CP - 1 staged
// as zeros.  Nothing beyond column n_channels - 1 of features, feature_map, grad_feature_map or grad_features is read
// or written.
template <int CP>
__device__ __forceinline__ void stage_features(const float* __restrict__ features, int C, const int* __restrict__ sorted,
                                               int first, int cnt, int tid, float* s_feat) {
    // by the whole workgroup: CP consecutive threads read the consecutive words of a row (as stage_chunk's coefficient
    // rows), RB / CP rows per step -- a thread keeps its channel and moves down the rows, four rows' loads in flight
    // before the first is stored (one row at a time was two dependent global latencies per step: 16 steps for 64
    // entries of 32 channels)
    constexpr int RPS = RB / CP;   // rows per step
    constexpr int U = 4;
    const int c = tid % CP, r0 = tid / CP;
    for (int rb = r0; rb < cnt; rb += U * RPS) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = rb + u * RPS;
            v[u] = (r < cnt && c < C) ? features[(size_t)sorted[first + r] * C + c] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = rb + u * RPS;
            if (r < cnt) s_feat[r * CP + c] = v[u];
        }
    }
}

template <int CP>
struct FeatureRows {
    static_assert(CP % 4 == 0 && CP >= 4 && CP <= 32, "padded channel count");
    const float* __restrict__ features;
    int C;
    float* s_feat;   // [chunk entry][CP]
    __device__ __forceinline__ void stage(const int* __restrict__ sorted, int first, int cnt, int tid, float*,
                                          const int*) const {
        stage_features<CP>(features, C, sorted, first, cnt, tid, s_feat);
    }
    // whether the C-float rows of a [H, W, C] map are whole 16-byte words (workgroup-uniform): a quarter of the memory
    // instructions; at 32 channels the map is 128 bytes per pixel and the forward of a short-list frame is bound by
    // writing it
    __device__ __forceinline__ bool rows_of_vec4(const float* map) const {
        return (C & 3) == 0 && ((uintptr_t)map & 15) == 0;
    }
};

template <int CP>
struct FeaturesFwd : FeatureRows<CP> {
    float* __restrict__ fmap;
    static constexpr int N = CP;
    __device__ __forceinline__ void add(float (&F)[CP], float w, const float*, int i, float) const {
        const Vec4<float>* f4 = reinterpret_cast<const Vec4<float>*>(this->s_feat + i * CP);
#pragma unroll
        for (int c4 = 0; c4 < CP / 4; c4++) {
            const Vec4<float> f = f4[c4];
            F[4 * c4 + 0] = __builtin_fmaf(w, f.x, F[4 * c4 + 0]);
            F[4 * c4 + 1] = __builtin_fmaf(w, f.y, F[4 * c4 + 1]);
            F[4 * c4 + 2] = __builtin_fmaf(w, f.z, F[4 * c4 + 2]);
            F[4 * c4 + 3] = __builtin_fmaf(w, f.w, F[4 * c4 + 3]);
        }
    }
    __device__ __forceinline__ void store(const float (&F)[CP], size_t p) const {
        const int C = this->C;
        float* row = fmap + p * C;
        if (this->rows_of_vec4(fmap)) {
#pragma unroll
            for (int c4 = 0; c4 < CP / 4; c4++) {
                if (4 * c4 < C) {
                    Vec4<float> v4;
                    v4.x = F[4 * c4 + 0]; v4.y = F[4 * c4 + 1]; v4.z = F[4 * c4 + 2]; v4.w = F[4 * c4 + 3];
                    reinterpret_cast<Vec4<float>*>(row)[c4] = v4;
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < CP; c++)
                if (c < C) row[c] = F[c];
        }
    }
};

// c_k = g_alpha + sum_c g[c] f_k[c] (a fused multiply-add chain from g_alpha, channels ascending); the slot's sum 0
// stays zero.  The feature gradient dL/df[k, c] = sum_pixels w_k(p) g[p, c] does not go through the slots: per wave it
// is the contraction [channels x 64 pixels] x [64 pixels x 16 entries], done with v_mfma_f32_16x16x4_f32 (exact fp32)
// on batches of 16 contributing entries as k_render_bwd_sh contracts its coefficient gradients -- the pixel-side
// operand g[pixel][channel] stays in registers for the whole walk (y_op, one set of 16 per block of 16 channels), the
// entries' w_k go to the wave's LDS batch, two accumulator chains per channel block, and the results are added
// straight to grad_features rows, consecutive lanes on consecutive words of a row.  A batch stays open across chunks
// (it keeps the Gaussian indices itself) and the partial one is flushed at the end of the walk.
// grad_features == nullptr: none of it runs.
template <int CP>
struct FeaturesBwd : FeatureRows<CP> {
    static constexpr int MB = 16;               // entries per MFMA batch (the N of 16x16x4)
    static constexpr int BROW = 64 + 4;         // floats per row of the batch's weight matrix [slot][pixel]
    static constexpr int NBLK = (CP + 15) / 16; // blocks of 16 channels (the M of 16x16x4)
    static constexpr int OW = 16 * NBLK;        // floats per slot of the batch's result [slot][channel]
    static_assert(64 * 17 <= MB * BROW && MB * OW <= MB * BROW, "scratch uses of the wave's batch rows");
    const float* __restrict__ g_map;
    float* __restrict__ grad_features;   // nullptr: no batch runs
    float* mine;                         // s_B, from begin() the wave's rows of it: [slot][pixel] w of the open batch
    int* bidx;                           // s_bidx, the wave's row of it: [slot] Gaussian index of the entry
    int lane = 0;
    bool want_f = false;   // grad_features != nullptr (workgroup-uniform)
    float g[CP] = {};
    float y_op[NBLK][16] = {};
    int nb = 0;   // filled slots of the wave's open batch (wave-uniform)

    __device__ __forceinline__ void load(size_t p) {
        const int C = this->C;
        if (g_map == nullptr) return;
        if (this->rows_of_vec4(g_map)) {
#pragma unroll
            for (int c4 = 0; c4 < CP / 4; c4++) {
                if (4 * c4 < C) {
                    const Vec4<float> v4 = reinterpret_cast<const Vec4<float>*>(g_map + p * C)[c4];
                    g[4 * c4 + 0] = v4.x; g[4 * c4 + 1] = v4.y; g[4 * c4 + 2] = v4.z; g[4 * c4 + 3] = v4.w;
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < CP; c++)
                if (c < C) g[c] = g_map[p * C + c];
        }
    }
    // The batch GEMM per block of 16 channels  D[c][j] = sum_k A[c][k] B[k][j]  with  A[c][k] = g[pixel k][channel c]
    // (constant over the walk) and B[k][j] = w of batch slot j at pixel k.  As in k_render_bwd_sh the contraction index
    // of MFMA step t, sub-index q (= lane >> 4) is pixel 16 q + t of the wave, so that lane 16 q + j finds its sixteen
    // B values (slot j, pixels 16 q .. 16 q + 15) contiguous in LDS:  y_op[blk][t] = g[pixel 16 q + t][16 blk + (lane & 15)]
    __device__ __forceinline__ void begin(int lane_, int wave) {
        lane = lane_;
        want_f = grad_features != nullptr;
        mine += wave * MB * BROW;
        bidx += wave * MB;
        if (!want_f) return;
#pragma unroll
        for (int blk = 0; blk < NBLK; blk++) {
            // the wave's batch rows as [pixel][17] for the transposition
#pragma unroll
            for (int s2 = 0; s2 < 16; s2++)
                mine[lane * 17 + s2] = (16 * blk + s2 < CP) ? g[(16 * blk + s2 < CP) ? 16 * blk + s2 : 0] : 0.0f;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int t = 0; t < 16; t++) y_op[blk][t] = mine[(16 * (lane >> 4) + t) * 17 + (lane & 15)];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    __device__ __forceinline__ float c(float ga, const Vec4<float>&, int i, float, float, float) const {
        float c = ga;
        const Vec4<float>* f4 = reinterpret_cast<const Vec4<float>*>(this->s_feat + i * CP);
#pragma unroll
        for (int c4 = 0; c4 < CP / 4; c4++) {
            const Vec4<float> f = f4[c4];
            c = __builtin_fmaf(g[4 * c4 + 0], f.x, c);
            c = __builtin_fmaf(g[4 * c4 + 1], f.y, c);
            c = __builtin_fmaf(g[4 * c4 + 2], f.z, c);
            c = __builtin_fmaf(g[4 * c4 + 3], f.w, c);
        }
        return c;
    }
    __device__ __forceinline__ float column0(float) const { return 0.0f; }
    // column nb of the batch's B: this entry's w at the wave's 64 pixels (0 where it does not contribute)
    __device__ __forceinline__ void visited(float aT, int g_index) {
        if (!want_f) return;
        mine[nb * BROW + lane] = aT;
        if (lane == 0) bidx[nb] = g_index;
        if (++nb == MB) {
            mma_flush(MB);
            nb = 0;
        }
    }
    __device__ __forceinline__ void send(int, int, float) const {}
    __device__ __forceinline__ void finish() {
        if (nb > 0) mma_flush(nb);   // the partial batch
    }
    // The GEMM of the open batch; its results are the wave's complete sums for (tile patch, entry) and go straight to
    // the global gradient rows
    __device__ __forceinline__ void mma_flush(int n_filled) {
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        const int C = this->C;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int j = lane & 15, q = lane >> 4;
        const Vec4<float>* brow = reinterpret_cast<const Vec4<float>*>(mine + j * BROW + 16 * q);
        float b[16];
#pragma unroll
        for (int m4 = 0; m4 < 4; m4++) {
            const Vec4<float> v4 = brow[m4];
            b[4 * m4 + 0] = v4.x; b[4 * m4 + 1] = v4.y; b[4 * m4 + 2] = v4.z; b[4 * m4 + 3] = v4.w;
        }
        f32x4 acc[NBLK];
#pragma unroll
        for (int blk = 0; blk < NBLK; blk++) {
            f32x4 even = {0, 0, 0, 0}, odd = {0, 0, 0, 0};   // two chains: the dependent-issue latency is 40 cycles
#pragma unroll
            for (int t = 0; t < 16; t += 2) {
                even = __builtin_amdgcn_mfma_f32_16x16x4f32(y_op[blk][t], b[t], even, 0, 0, 0);
                odd = __builtin_amdgcn_mfma_f32_16x16x4f32(y_op[blk][t + 1], b[t + 1], odd, 0, 0, 0);
            }
            acc[blk] = even + odd;
        }
        // D: column j = lane & 15 (the batch slot), rows c = 4 q + r  ->  the wave's scratch as [slot][OW]
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();   // every lane has read its B values
#pragma unroll
        for (int blk = 0; blk < NBLK; blk++) {
            Vec4<float> v4;
            v4.x = acc[blk][0]; v4.y = acc[blk][1]; v4.z = acc[blk][2]; v4.w = acc[blk][3];
            *reinterpret_cast<Vec4<float>*>(mine + j * OW + blk * 16 + 4 * q) = v4;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // consecutive lanes, consecutive words of a gradient row
        for (int k = lane; k < n_filled * CP; k += 64) {
            const int row = k / CP, c = k - row * CP;
            if (c < C) global_add(grad_features + (size_t)bidx[row] * C + c, mine[row * OW + c]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

// LDS: 12 KB of records + CP KB of feature rows.
template <int CP>
__global__ __launch_bounds__(RB) void k_render_features_fwd(
    const float* __restrict__ packed, const float* __restrict__ features, int C, const int* __restrict__ ranges,
    const int* __restrict__ sorted, const int* __restrict__ nsp_in, int W, int H, int ntx, int tile0, int nt,
    float* __restrict__ fmap, float* __restrict__ alpha_out, float* __restrict__ t_out) {
    __shared__ alignas(16) float s_geom[MAP_FWD_CHUNK * GS_PACKED_WIDTH];
    __shared__ alignas(16) float s_feat[MAP_FWD_CHUNK * CP];
    __shared__ unsigned long long s_mask[4][MAP_FWD_CHUNK / 64];
    __shared__ int s_max[4];
    FeaturesFwd<CP> ch{{features, C, s_feat}, fmap};
    render_map_fwd(ch, packed, ranges, sorted, nsp_in, W, H, ntx, tile0, nt, alpha_out, t_out, s_geom, s_mask, s_max);
}

// LDS: 3 KB records + CP / 4 KB feature rows + 9 KB slots + 17 KB batches.
template <int CP>
__global__ __launch_bounds__(RB) void k_render_features_bwd(
    const float* __restrict__ packed, const float* __restrict__ features, int C, const int* __restrict__ ranges,
    const int* __restrict__ sorted, const int* __restrict__ nsp_in, const float* __restrict__ t_in,
    const float* __restrict__ g_map, const float* __restrict__ g_alpha, int W, int H, int ntx, int tile0, int nt,
    float* __restrict__ slab, float* __restrict__ grad_features) {
    using Ch = FeaturesBwd<CP>;
    __shared__ alignas(16) float s_geom[MAP_BWD_CHUNK * GS_PACKED_WIDTH];
    __shared__ alignas(16) float s_feat[MAP_BWD_CHUNK * CP];
    __shared__ int s_idx[MAP_BWD_CHUNK];
    __shared__ float s_acc[4 * MAP_BWD_CHUNK * 9];            // [wave][entry][9]
    __shared__ alignas(16) float s_B[4 * Ch::MB * Ch::BROW];  // [wave][slot][pixel]
    __shared__ int s_bidx[4 * Ch::MB];                        // [wave][slot]
    __shared__ int s_max[4];
    __shared__ unsigned long long s_mask[4][1];
    __shared__ unsigned long long s_hit[4][1];                // slots written by each wave
    Ch ch{{features, C, s_feat}, g_map, grad_features, s_B, s_bidx};
    render_map_bwd(ch, packed, ranges, sorted, nsp_in, t_in, g_alpha, W, H, ntx, tile0, nt, slab, s_geom, s_idx, s_acc,
                   s_max, s_mask, s_hit);
}

// ---------------------------------------------------------------------------------------------------
// per-Gaussian contribution statistics (no reference counterpart), fp32, forward only
// ---------------------------------------------------------------------------------------------------
// The blending weights w_k = alpha_k T_k of the frame whose colour forward left num_splats_per_pixel, reduced over the
// pixels per Gaussian instead of over the Gaussians per pixel: their sum, their largest and the number of pixels.  alpha,
// the contribute decision and T are the depth kernel's (zalpha_alpha; w = alpha T, T = fma(-alpha, T, T)), so a weight
// here has the bits of k_render_zalpha_fwd's.  The kernel has its OWN walk body (render_map_fwd keeps its ISA): front to
// back with T in a register like the forward, but with the backward's exchange -- per visited entry the wave reduces over
// its patch's pixels (lanes that do not contribute hold 0) and leaves the result in the wave's own LDS slot of the
// entry, plain stores; s_hit marks the slots a wave wrote; after the chunk thread = staged entry combines the four
// waves' slots in wave order and sends at most three global atomics to the Gaussian's row.
//   count  popcount of the ballot of `contrib`: scalar, no lane traffic
//   sum, max   four DPP steps inside the 16-lane rows (xor 1, xor 2, row_ror 4, row_ror 8: every lane holds its row's
//          total), then rows -> wave for BOTH values with the two swaps of reduce9_to_slot: permlane16_swap(sum, max)
//          pairs the rows -- the sums of row pairs (0,1), (2,3) land in rows 0, 2, the maxima in rows 1, 3 -- and
//          permlane32_swap joins the halves.  Rows 0 / 2 add, rows 1 / 3 take the maximum (one select each): lane 0
//          ends with the wave's sum ((r0 + r1) + (r2 + r3), a fixed order), lane 16 with its maximum.
//   slot   three words per (wave, entry): sum | max | count.  Lanes 0, 16 and 32 store them with ONE ds_write_b32 (lane
//          32 carries the count's bits).  A pitch of three words is odd: the flush's reads, thread t at word 3 t, are
//          free of bank conflicts.
// The maximum goes out as a signed integer atomic on the float's bits: the weights are positive (alpha >= 1/255, T > 0),
// where the order of the bits is the order of the values, so the result does not depend on the order of the tiles.
// RCHUNK entries are staged per step (GS_CONTRIB_CHUNK; gs_debug_contributions_chunk selects the other instantiation
// for the measurement, scripts/contributions_cost.py).
// (dpp_lanes: with the wave reductions, in front of the backward kernels)
// the maximum's bits where the lane's mask is set, the sum elsewhere: one select on a mask formed before the walk (with
// `odd_row ? max : sum` the compiler puts each value into an exec-masked branch of its own)
__device__ __forceinline__ float row_select(unsigned mask, unsigned max_bits, float sum) {
    return __uint_as_float((max_bits & mask) | (__float_as_uint(sum) & ~mask));
}
constexpr int CONTRIB_SLOT = 3;   // words per (wave, entry) slot: sum | max | count

template <int RCHUNK>
__global__ __launch_bounds__(RB) void k_render_contrib(
    const float* __restrict__ packed, const int* __restrict__ ranges, const int* __restrict__ sorted,
    const int* __restrict__ nsp_in, const int* __restrict__ row_index, int W, int H, int ntx, int tile0, int nt,
    float* __restrict__ weight_sum, int* __restrict__ weight_max_bits, int* __restrict__ pixel_count) {
    constexpr int NW = RCHUNK / 64;
    constexpr int SV = CONTRIB_SLOT;
    __shared__ alignas(16) float s_geom[RCHUNK * GS_PACKED_WIDTH];
    __shared__ int s_idx[RCHUNK];
    __shared__ int s_slot[4 * RCHUNK * SV];          // [wave][entry][sum | max | count], the floats as their bits
    __shared__ int s_max[4];
    __shared__ unsigned long long s_mask[4][NW];
    __shared__ unsigned long long s_hit[4][NW];      // slots written by each wave
    const int t_local = tile_of_block(blockIdx.x, nt);
    if (t_local >= nt) return;
    const int tile = tile0 + t_local;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    const bool valid = px.u < W && px.v < H;
    const int s0 = ranges[tile];
    const int n_tile = ranges[tile + 1] - s0;
    const int nsp = valid ? nsp_in[(size_t)px.v * W + px.u] : 0;
    int n_used, wave_used;
    zalpha_reach(nsp, n_tile, tid, s_max, n_used, wave_used);
    if (n_used <= 0) return;
    const float pu = float(px.u), pv = float(px.v);
    const unsigned odd_mask = (lane & 16) != 0 ? ~0u : 0u;         // rows 1, 3 carry the maximum, rows 0, 2 the sum
    const bool slot_stores = (lane & 15) == 0 && lane < 48;        // lanes 0, 16, 32: sum, max, count
    const int slot_lane_base = wave * RCHUNK * SV + (lane >> 4);   // (lane 48: word 3 = the next entry's, never stored)
    float T = 1.0f;
    for (int base = 0; base < n_used; base += RCHUNK) {
        const int cnt = min(RCHUNK, n_used - base);
        if (base > 0) __syncthreads();   // the previous chunk is flushed
        stage_chunk<float, 1>(packed, nullptr, sorted, s0 + base, cnt, tid, s_geom, nullptr, s_idx);
        if (lane < NW) s_hit[wave][lane] = 0;   // (the wave's own words; a wave that stops early leaves them so)
        // (no barrier in between: thread t tests the record thread t staged)
        build_touch_masks<float, RCHUNK>(s_geom, cnt, tid, tile % ntx, tile / ntx, s_mask);
        __syncthreads();
        for (int word = 0; word < NW && word * 64 < cnt; word++) {
            if (base + word * 64 >= wave_used) break;   // wave-uniform: no pixel of the patch walked this far
            unsigned long long m = wave_uniform(s_mask[wave][word]);
            unsigned long long hit = 0;   // the entries of this word whose slot the wave wrote
            while (m) {
                const int b = __builtin_ctzll(m);
                const int i = word * 64 + b;
                m &= m - 1;
                const int k = base + i;
                if (k >= wave_used) break;
                const float* rec = s_geom + i * GS_PACKED_WIDTH;
                const Vec4<float> g0 = *reinterpret_cast<const Vec4<float>*>(rec);       // u v r2 opacity
                const Vec4<float> g1 = *reinterpret_cast<const Vec4<float>*>(rec + 4);   // a b c det
                const ZalphaVisit v = zalpha_alpha(g0, g1, rec[8], pu, pv, k < nsp);
                const unsigned long long bal = ballot(v.contrib);
                if (bal == 0) continue;   // every reaching lane skipped the entry
                float w = 0.0f;
                if (v.contrib) {
                    w = v.alpha * T;
                    T = __builtin_fmaf(-v.alpha, T, T);   // T (1 - alpha), one rounding
                }
                // rows: every lane ends with its row's sum and maximum.  The maximum is taken on the bits as unsigned
                // integers (w >= 0: the same order; v_max_u32 takes the DPP operand directly and 0 is its identity, where
                // v_max_f32 first canonicalises both operands)
                float sum = w;
                unsigned mxb = __float_as_uint(w);
                sum += dpp_lanes<0xB1>(sum);  mxb = max(mxb, dpp_lanes<0xB1>(mxb));    // quad_perm [1,0,3,2]
                sum += dpp_lanes<0x4E>(sum);  mxb = max(mxb, dpp_lanes<0x4E>(mxb));    // quad_perm [2,3,0,1]
                sum += dpp_lanes<0x124>(sum); mxb = max(mxb, dpp_lanes<0x124>(mxb));   // row_ror:4
                sum += dpp_lanes<0x128>(sum); mxb = max(mxb, dpp_lanes<0x128>(mxb));   // row_ror:8
                // rows -> wave
                float mx = __uint_as_float(mxb);
                permlane16_swap(sum, mx);        // sum: rows (s0, m0, s2, m2); mx: rows (s1, m1, s3, m3)
                float z = row_select(odd_mask, max(__float_as_uint(sum), __float_as_uint(mx)), sum + mx);
                float z2 = z;
                permlane32_swap(z, z2);          // z: rows 0, 1 twice; z2: rows 2, 3 twice
                const float total = row_select(odd_mask, max(__float_as_uint(z), __float_as_uint(z2)), z + z2);
                const int out = lane == 32 ? (int)__builtin_popcountll(bal) : __float_as_int(total);
                int slot_i = i * SV;
                asm volatile("" : "+s"(slot_i));
                if (slot_stores) s_slot[slot_lane_base + slot_i] = out;
                hit |= 1ull << b;
            }
            if (lane == 0) s_hit[wave][word] = hit;
        }
        __syncthreads();
        // thread = staged entry: the waves' slots in wave order, then one atomic per output to the Gaussian's row
        if (tid < cnt) {
            float sum = 0.0f;
            unsigned mxb = 0;   // (the bits of 0.0f)
            int n = 0;
#pragma unroll
            for (int w4 = 0; w4 < 4; w4++) {
                if ((s_hit[w4][tid >> 6] >> (tid & 63)) & 1ull) {
                    const int* sl = s_slot + (w4 * RCHUNK + tid) * SV;
                    sum += __int_as_float(sl[0]);
                    mxb = max(mxb, (unsigned)sl[1]);
                    n += sl[2];
                }
            }
            if (n > 0) {
                const int g = s_idx[tid];
                const size_t r = row_index != nullptr ? (size_t)row_index[g] : (size_t)g;
                if (weight_sum != nullptr) global_add(weight_sum + r, sum);
                if (weight_max_bits != nullptr) atomicMax(weight_max_bits + r, (int)mxb);
                if (pixel_count != nullptr) atomicAdd(pixel_count + r, n);
            }
        }
    }
}

}  // namespace gs

using namespace gs;

#define DISPATCH_T(dtype, CALL)                                                                    \
    if ((dtype) == GS_F32) {                                                                       \
        using T = float;                                                                           \
        CALL;                                                                                      \
    } else if ((dtype) == GS_F64) {                                                                \
        using T = double;                                                                          \
        CALL;                                                                                      \
    } else {                                                                                       \
        gs::set_error("Inputs must be float32 or float64");                                        \
        return GS_EINVAL;                                                                          \
    }

#define DISPATCH_SH(n_sh, CALL)                                                                    \
    switch (n_sh) {                                                                                \
        case 1: { constexpr int N_SH = 1; CALL; } break;                                           \
        case 4: { constexpr int N_SH = 4; CALL; } break;                                           \
        case 9: { constexpr int N_SH = 9; CALL; } break;                                           \
        case 16: { constexpr int N_SH = 16; CALL; } break;                                         \
        default:                                                                                   \
            gs::set_error("Unsupported number of SH coefficients: %d", n_sh);                      \
            return GS_EINVAL;                                                                      \
    }

// the feature kernels' instantiation at or above n_channels (checked to be in 1..32): CP = 4, 8, 16, 32
#define DISPATCH_CP(n_channels, CALL)                                                              \
    if ((n_channels) <= 4) { constexpr int CP = 4; CALL; }                                         \
    else if ((n_channels) <= 8) { constexpr int CP = 8; CALL; }                                    \
    else if ((n_channels) <= 16) { constexpr int CP = 16; CALL; }                                  \
    else { constexpr int CP = 32; CALL; }

static int check_rows(int H, int row0, int row1) {
    const int nty = (H + 15) / 16;
    if (row0 < 0 || row1 > nty || row0 > row1) {
        gs::set_error("bad tile row range [%d, %d) for %d tile rows", row0, row1, nty);
        return GS_EINVAL;
    }
    return GS_OK;
}

// process-wide DEFAULT of the render backward's gradient mode; every entry point takes the mode per call
// (ABI 5) and reads this only when asked for GS_BACKWARD_DEFAULT, once, at the call
static std::atomic<int> g_backward_mode{GS_BACKWARD_COMPAT};
static int resolve_backward_mode(int mode, int* exact) {
    if (mode == GS_BACKWARD_DEFAULT) mode = g_backward_mode.load(std::memory_order_relaxed);
    if (mode != GS_BACKWARD_COMPAT && mode != GS_BACKWARD_EXACT) {
        gs::set_error("backward mode must be GS_BACKWARD_DEFAULT, GS_BACKWARD_COMPAT or GS_BACKWARD_EXACT");
        return GS_EINVAL;
    }
    *exact = mode == GS_BACKWARD_EXACT;
    return GS_OK;
}

// the general forward of one (dtype, coefficient count).  fp32 with one coefficient never gets here (launch_render_fwd
// launches the fused kernel itself), but DISPATCH_SH names that pair too and k_render_fwd_general refuses it
template <typename T, int N_SH>
static void launch_render_fwd_general(hipStream_t s, int grid, const void* packed_or_uvs, const void* opacity,
                                      const void* conic, const void* rgb, const void* view_dir, const int* ranges,
                                      const int* sorted, const void* bg, int W, int H, int ntx, int tile0, int nt,
                                      int* nsp_out, void* fw_out, void* image) {
    if constexpr (!(sizeof(T) == 4 && N_SH == 1))
        k_render_fwd_general<T, N_SH><<<grid, RB, 0, s>>>(
            (const T*)packed_or_uvs, (const T*)rgb, (const T*)view_dir, ranges, sorted, (const T*)bg, W, H, ntx, tile0,
            nt, nsp_out, (T*)fw_out, (T*)image, (const T*)opacity, (const T*)conic);
}

extern "C" {

int gs_set_backward_mode(int mode) {
    GS_REQUIRE(mode == GS_BACKWARD_COMPAT || mode == GS_BACKWARD_EXACT, "backward mode must be GS_BACKWARD_COMPAT or GS_BACKWARD_EXACT");
    g_backward_mode.store(mode, std::memory_order_relaxed);
    return GS_OK;
}
int gs_get_backward_mode(void) { return g_backward_mode.load(std::memory_order_relaxed); }

#ifdef GS_STATS
// instrumented build only: copies the 32 counters to the host (and clears them when reset != 0)
int gs_debug_render_stats(unsigned long long* out, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return GS_EHIP;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gs::g_render_stats), 32 * sizeof(unsigned long long)) != hipSuccess)
        return GS_EHIP;
    if (reset) {
        unsigned long long z[32] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(gs::g_render_stats), z, sizeof(z)) != hipSuccess) return GS_EHIP;
    }
    return GS_OK;
}
// instrumented build only: copies the wave timeline (2 kernels x GS_TIMELINE_CAP slots x GS_TIMELINE_W u64; unused
// slots are zero) to the host and clears it
int gs_debug_render_timeline(unsigned long long* out, int cap_waves) {
    if (hipDeviceSynchronize() != hipSuccess) return GS_EHIP;
    if (cap_waves != gs::GS_TIMELINE_CAP) return GS_EINVAL;
    const size_t bytes = (size_t)2 * gs::GS_TIMELINE_CAP * gs::GS_TIMELINE_W * sizeof(unsigned long long);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gs::g_timeline), bytes) != hipSuccess) return GS_EHIP;
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(gs::g_timeline)) != hipSuccess) return GS_EHIP;
    if (hipMemset(p, 0, bytes) != hipSuccess) return GS_EHIP;
    return GS_OK;
}
#endif

static int launch_render_fwd(const void* packed_or_uvs, const void* opacity, const void* conic, const void* rgb,
                             const void* view_dir_by_pixel, const int32_t* tile_ranges,
                             const int32_t* sorted_gaussians, const void* background_rgb, int W, int H, int n_sh,
                             int tile_row0, int tile_row1, int32_t* num_splats_per_pixel,
                             void* final_weight_per_pixel, void* image, int dtype, void* stream,
                             void* segment_state = nullptr) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    if (int e = check_rows(H, tile_row0, tile_row1)) return e;
    hipStream_t s = (hipStream_t)stream;
    const int ntx = (W + 15) / 16;
    const int nt = (tile_row1 - tile_row0) * ntx;
    if (nt == 0) return GS_OK;
    const int grid = render_grid(nt);
    if (segment_state != nullptr) {   // the fused renderer's kernel with the state for the segmented backward
        GS_REQUIRE(dtype == GS_F32 && n_sh == 1 && opacity == nullptr,
                   "segment_state needs float32 packed records and one colour coefficient per channel");
        GS_REQUIRE(((uintptr_t)segment_state & 15) == 0, "segment_state must be 16-byte aligned");
        k_render_fwd_ck<<<grid, RB, 0, s>>>(
            (const float*)packed_or_uvs, (const float*)rgb, tile_ranges, sorted_gaussians,
            (const float*)background_rgb, W, H, ntx, tile_row0 * ntx, nt, num_splats_per_pixel,
            (float*)final_weight_per_pixel, (float*)image, 0, nullptr, INT64_MAX, nullptr,
            seg_state_of(segment_state, W, H, tile_row0, tile_row1), nullptr);
        return check_launch("render_tiles");
    }
    if (dtype == GS_F32 && n_sh == 1) {   // the fused renderer's kernel on whole lists: no prefix, flags, cost or hand-over
        k_render_fwd<float, 1><<<grid, RB, 0, s>>>(
            (const float*)packed_or_uvs, (const float*)rgb, nullptr, tile_ranges, sorted_gaussians,
            (const float*)background_rgb, W, H, ntx, tile_row0 * ntx, nt, num_splats_per_pixel,
            (float*)final_weight_per_pixel, (float*)image, 0, nullptr, INT64_MAX, nullptr, (const float*)opacity,
            (const float*)conic, nullptr, nullptr, nullptr);
        return check_launch("render_tiles");
    }
    DISPATCH_T(dtype, DISPATCH_SH(n_sh, (launch_render_fwd_general<T, N_SH>(
                                            s, grid, packed_or_uvs, opacity, conic, rgb, view_dir_by_pixel, tile_ranges,
                                            sorted_gaussians, background_rgb, W, H, ntx, tile_row0 * ntx, nt,
                                            num_splats_per_pixel, final_weight_per_pixel, image))));
    return check_launch("render_tiles");
}

int gs_render_tiles(const void* uvs, const void* opacity, const void* rgb, const void* conic,
                    const void* view_dir_by_pixel, const int32_t* tile_ranges,
                    const int32_t* sorted_gaussians, const void* background_rgb,
                    int32_t* num_splats_per_pixel, void* final_weight_per_pixel, void* image, int W, int H,
                    int n_sh, int tile_row0, int tile_row1, int dtype, void* stream) {
    GS_REQUIRE(opacity != nullptr && conic != nullptr, "opacity and conic must not be null");
    return launch_render_fwd(uvs, opacity, conic, rgb, view_dir_by_pixel, tile_ranges, sorted_gaussians,
                             background_rgb, W, H, n_sh, tile_row0, tile_row1, num_splats_per_pixel,
                             final_weight_per_pixel, image, dtype, stream);
}

int gs_render_tiles_packed(const void* packed, const void* rgb, const void* view_dir_by_pixel,
                           const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                           const void* background_rgb, int W, int H, int n_sh, int tile_row0,
                           int tile_row1, int32_t* num_splats_per_pixel, void* final_weight_per_pixel,
                           void* image, int dtype, void* segment_state, void* stream) {
    return launch_render_fwd(packed, nullptr, nullptr, rgb, view_dir_by_pixel, tile_ranges, sorted_gaussians,
                             background_rgb, W, H, n_sh, tile_row0, tile_row1, num_splats_per_pixel,
                             final_weight_per_pixel, image, dtype, stream, segment_state);
}

size_t gs_render_segment_workspace_bytes(int W, int H, int tile_row0, int tile_row1) {
    if (W <= 0 || H <= 0 || tile_row0 < 0 || tile_row1 <= tile_row0 || tile_row1 > (H + 15) / 16) return 0;
    const size_t Tb = (size_t)((W + 15) / 16) * (size_t)(tile_row1 - tile_row0);
    return Tb * SEG_MAX * 256 * sizeof(Vec4<float>) + seg_band_pixels(W, H, tile_row0, tile_row1) * 12;
}

int gs_render_tiles_prefix(const void* packed, const void* rgb, const int32_t* tile_ranges,
                           int32_t* sorted_gaussians, const uint64_t* keys, int64_t S,
                           const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                           int32_t* tile_flags, int32_t* num_splats_per_pixel,
                           void* final_weight_per_pixel, void* image, int32_t* tile_cost, void* segment_state,
                           void* stream) {
    return gs_render_tiles_prefix_phased(packed, rgb, tile_ranges, sorted_gaussians, keys, S, background_rgb, W, H, tile_row0,
                                         tile_row1, tile_flags, num_splats_per_pixel, final_weight_per_pixel, image,
                                         tile_cost, segment_state, GS_PREFIX_RENDER | GS_PREFIX_REPAIR, stream);
}

int gs_render_tiles_prefix_phased_m(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                  int32_t* sorted_gaussians, const uint64_t* keys, int64_t S,
                                  const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                                  int32_t* tile_flags, int32_t* num_splats_per_pixel, void* final_weight_per_pixel,
                                  void* image, int32_t* tile_cost, void* segment_state, int phases, uint64_t* touch_masks, void* stream) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    GS_REQUIRE(phases >= 1 && phases <= 3, "phases: GS_PREFIX_RENDER, GS_PREFIX_REPAIR or both");
    GS_REQUIRE(tile_flags != nullptr, "tile_flags must not be null");
    GS_REQUIRE(segment_state == nullptr || ((uintptr_t)segment_state & 15) == 0, "segment_state must be 16-byte aligned");
    if (int e = check_rows(H, tile_row0, tile_row1)) return e;
    hipStream_t s = (hipStream_t)stream;
    const int ntx = (W + 15) / 16;
    const int nt = (tile_row1 - tile_row0) * ntx;
    if (nt == 0) return GS_OK;
    const int grid = render_grid(nt);
    const int t0 = tile_row0 * ntx;
    const SegState seg = seg_state_of(segment_state, W, H, tile_row0, tile_row1);
    // 1. provisional pass over the ordered prefixes; raises the flags
    if (phases & GS_PREFIX_RENDER) {
        if (segment_state)
            k_render_fwd_ck<<<grid, RB, 0, s>>>(
                (const float*)packed, (const float*)rgb, tile_ranges, sorted_gaussians, (const float*)background_rgb, W, H,
                ntx, t0, nt, num_splats_per_pixel, (float*)final_weight_per_pixel, (float*)image, GS_SORT_PREFIX,
                tile_flags, S, tile_cost, seg, (unsigned long long*)touch_masks);
        else
            k_render_fwd<float, 1><<<grid, RB, GS_FWD_LDS_PAD, s>>>(
                (const float*)packed, (const float*)rgb, nullptr, tile_ranges, sorted_gaussians,
                (const float*)background_rgb, W, H, ntx, t0, nt, num_splats_per_pixel,
                (float*)final_weight_per_pixel, (float*)image, GS_SORT_PREFIX, tile_flags, S, tile_cost, nullptr, nullptr,
                nullptr, nullptr, (unsigned long long*)touch_masks);
    }
    if ((phases & GS_PREFIX_REPAIR) && S > GS_SORT_PREFIX) {
        // 2. flagged tiles: full sort + render again, one launch (exits at once on a dense scene)
        const size_t lds = sort_lds_bytes(S <= 4096 ? 4096 : SORT_MAX_LDS_KEYS);
        const auto repair = segment_state ? launch_render_fwd_flagged<true> : launch_render_fwd_flagged<false>;
        repair(s, lds, packed, rgb, tile_ranges, sorted_gaussians, background_rgb, W, H, ntx, t0, nt, num_splats_per_pixel,
               final_weight_per_pixel, image, tile_flags, S, tile_cost, seg, nullptr, nullptr,
               const_cast<uint64_t*>(keys), GS_SORT_PREFIX, 0, touch_masks);
    }
    return check_launch("render_tiles_prefix");
}

int gs_render_tiles_prefix_phased(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                  int32_t* sorted_gaussians, const uint64_t* keys, int64_t S,
                                  const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                                  int32_t* tile_flags, int32_t* num_splats_per_pixel, void* final_weight_per_pixel,
                                  void* image, int32_t* tile_cost, void* segment_state, int phases, void* stream) {
    return gs_render_tiles_prefix_phased_m(packed, rgb, tile_ranges, sorted_gaussians, keys, S, background_rgb, W, H, tile_row0,
                                           tile_row1, tile_flags, num_splats_per_pixel, final_weight_per_pixel, image, tile_cost,
                                           segment_state, phases, nullptr, stream);
}

// the fused renderer's forward on depth-cut lists (binning.hip "depth cut"; gs_tile_count_cut / gs_tile_emit_sort_cut)
int gs_render_tiles_cut_m(const void* packed, const void* rgb, const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                        int64_t S, const int32_t* full_ranges, const void* bin_records, int N, float mh_dist,
                        int32_t* workspace, int32_t* cut_workspace, uint64_t* overflow_keys, int32_t* overflow_sorted,
                        int64_t overflow_capacity, const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                        int32_t* tile_flags, int32_t* num_splats_per_pixel, void* final_weight_per_pixel, void* image,
                        int32_t* tile_cost, int32_t* host_flagged, uint64_t* touch_masks, void* stream) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    GS_REQUIRE(tile_flags != nullptr && full_ranges != nullptr, "tile_flags and full_ranges must not be null");
    if (int e = check_rows(H, tile_row0, tile_row1)) return e;
    hipStream_t s = (hipStream_t)stream;
    const int ntx = (W + 15) / 16, nty = (H + 15) / 16;
    const int nt = (tile_row1 - tile_row0) * ntx;
    if (nt == 0) return GS_OK;
    const int grid = render_grid(nt);
    const int t0 = tile_row0 * ntx;
    int* flag_counter = depth_cut_flag_counter(cut_workspace, N, ntx * nty);
    // 1. every tile from its kept (completely sorted) depth prefix; raises the flags
    k_render_fwd<float, 1><<<grid, RB, GS_FWD_LDS_PAD, s>>>(
        (const float*)packed, (const float*)rgb, nullptr, tile_ranges, sorted_gaussians, (const float*)background_rgb, W, H,
        ntx, t0, nt, num_splats_per_pixel, (float*)final_weight_per_pixel, (float*)image, 0, tile_flags, S, tile_cost,
        nullptr, nullptr, full_ranges, flag_counter, (unsigned long long*)touch_masks);
    // 2. + 3. flagged tiles: complete lists into the overflow buffers; sorted and rendered again by one workgroup each
    // (both launches exit at once while the frame has no flagged tile)
    if (int e = depth_cut_repair((const float*)bin_records, N, ntx, nty, mh_dist, tile_row0, tile_row1, full_ranges, workspace,
                                 cut_workspace, overflow_keys, overflow_capacity, overflow_sorted, tile_flags, s, false))
        return e;
    launch_render_fwd_flagged<false>(s, sort_lds_bytes(SORT_MAX_LDS_KEYS), packed, rgb, full_ranges, overflow_sorted,
                                     background_rgb, W, H, ntx, t0, nt, num_splats_per_pixel, final_weight_per_pixel, image,
                                     tile_flags, overflow_capacity, tile_cost, SEG_NONE, flag_counter, host_flagged,
                                     overflow_keys, 0, 1, touch_masks);
    return check_launch("render_tiles_cut");
}

int gs_render_tiles_cut(const void* packed, const void* rgb, const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                        int64_t S, const int32_t* full_ranges, const void* bin_records, int N, float mh_dist,
                        int32_t* workspace, int32_t* cut_workspace, uint64_t* overflow_keys, int32_t* overflow_sorted,
                        int64_t overflow_capacity, const void* background_rgb, int W, int H, int tile_row0, int tile_row1,
                        int32_t* tile_flags, int32_t* num_splats_per_pixel, void* final_weight_per_pixel, void* image,
                        int32_t* tile_cost, int32_t* host_flagged, void* stream) {
    return gs_render_tiles_cut_m(packed, rgb, tile_ranges, sorted_gaussians, S, full_ranges, bin_records, N, mh_dist, workspace,
                                 cut_workspace, overflow_keys, overflow_sorted, overflow_capacity, background_rgb, W, H, tile_row0,
                                 tile_row1, tile_flags, num_splats_per_pixel, final_weight_per_pixel, image, tile_cost,
                                 host_flagged, nullptr, stream);
}

static int launch_render_bwd(const void* packed_or_uvs, const void* opacity, const void* conic, const void* rgb,
                             const void* view_dir_by_pixel, const int32_t* tile_ranges,
                             const int32_t* sorted_gaussians, const void* background_rgb,
                             const int32_t* num_splats_per_pixel, const void* final_weight_per_pixel,
                             const void* grad_image, int W, int H, int n_sh, int tile_row0, int tile_row1,
                             void* grad_rgb, void* grad_opacity, void* grad_uv, void* grad_conic, int dtype,
                             int backward_mode, void* stream) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    if (int e = check_rows(H, tile_row0, tile_row1)) return e;
    int exact = 0;
    if (int e = resolve_backward_mode(backward_mode, &exact)) return e;
    hipStream_t s = (hipStream_t)stream;
    const int ntx = (W + 15) / 16;
    const int nt = (tile_row1 - tile_row0) * ntx;
    if (nt == 0) return GS_OK;
    const int grid = render_grid(nt);
    if (dtype == GS_F32 && n_sh == 1) {
        // one coefficient: the fused renderer's kernel on separate arrays or packed records, whole lists, grid order
        k_render_bwd<float, 1><<<grid, RB, 0, s>>>(
            (const float*)packed_or_uvs, (const float*)rgb, (const float*)view_dir_by_pixel, tile_ranges,
            sorted_gaussians, (const float*)background_rgb, num_splats_per_pixel,
            (const float*)final_weight_per_pixel, (const float*)grad_image, W, H, ntx, tile_row0 * ntx, nt,
            (float*)grad_rgb, (float*)grad_opacity, (float*)grad_uv, (float*)grad_conic, 0, exact, nullptr,
            (const float*)opacity, (const float*)conic, SEG_NONE, nullptr, nullptr, nullptr, nullptr);
    } else if (dtype == GS_F32) {
        decltype(&k_render_bwd_sh<4>) kernel = nullptr;
        switch (n_sh) {
            case 4: kernel = k_render_bwd_sh<4>; break;
            case 9: kernel = k_render_bwd_sh<9>; break;
            case 16: kernel = k_render_bwd_sh<16>; break;
            default:
                gs::set_error("Unsupported number of SH coefficients: %d", n_sh);
                return GS_EINVAL;
        }
        kernel<<<grid, RB, 0, s>>>(
            (const float*)packed_or_uvs, (const float*)rgb, (const float*)view_dir_by_pixel, tile_ranges,
            sorted_gaussians, (const float*)background_rgb, num_splats_per_pixel,
            (const float*)final_weight_per_pixel, (const float*)grad_image, W, H, ntx, tile_row0 * ntx, nt,
            (float*)grad_rgb, (float*)grad_opacity, (float*)grad_uv, (float*)grad_conic, exact,
            (const float*)opacity, (const float*)conic);
    } else if (dtype == GS_F64) {
        using T = double;
        DISPATCH_SH(n_sh, (k_render_bwd_ref<N_SH><<<grid, RB, 0, s>>>(
                              (const T*)packed_or_uvs, (const T*)rgb, (const T*)view_dir_by_pixel, tile_ranges,
                              sorted_gaussians, (const T*)background_rgb, num_splats_per_pixel,
                              (const T*)final_weight_per_pixel, (const T*)grad_image, W, H, ntx, tile_row0 * ntx, nt,
                              (T*)grad_rgb, (T*)grad_opacity, (T*)grad_uv, (T*)grad_conic, exact, (const T*)opacity,
                              (const T*)conic)));
    } else {
        gs::set_error("Inputs must be float32 or float64");
        return GS_EINVAL;
    }
    return check_launch("render_tiles_backward");
}

int gs_render_tiles_backward(const void* uvs, const void* opacity, const void* rgb, const void* conic,
                             const void* view_dir_by_pixel, const int32_t* tile_ranges,
                             const int32_t* sorted_gaussians, const void* background_rgb,
                             const int32_t* num_splats_per_pixel, const void* final_weight_per_pixel,
                             const void* grad_image, void* grad_rgb, void* grad_opacity, void* grad_uv,
                             void* grad_conic, int W, int H, int n_sh, int tile_row0, int tile_row1, int dtype,
                             int backward_mode, void* stream) {
    GS_REQUIRE(opacity != nullptr && conic != nullptr, "opacity and conic must not be null");
    return launch_render_bwd(uvs, opacity, conic, rgb, view_dir_by_pixel, tile_ranges, sorted_gaussians,
                             background_rgb, num_splats_per_pixel, final_weight_per_pixel, grad_image, W, H, n_sh,
                             tile_row0, tile_row1, grad_rgb, grad_opacity, grad_uv, grad_conic, dtype, backward_mode,
                             stream);
}

int gs_render_tiles_backward_packed(const void* packed, const void* rgb, const void* view_dir_by_pixel,
                                    const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                                    const void* background_rgb, const int32_t* num_splats_per_pixel,
                                    const void* final_weight_per_pixel, const void* grad_image, int W,
                                    int H, int n_sh, int tile_row0, int tile_row1, void* grad_rgb,
                                    void* grad_opacity, void* grad_uv, void* grad_conic, int dtype,
                                    int backward_mode, void* stream) {
    return launch_render_bwd(packed, nullptr, nullptr, rgb, view_dir_by_pixel, tile_ranges, sorted_gaussians,
                             background_rgb, num_splats_per_pixel, final_weight_per_pixel, grad_image, W, H, n_sh,
                             tile_row0, tile_row1, grad_rgb, grad_opacity, grad_uv, grad_conic, dtype, backward_mode,
                             stream);
}

static int launch_bwd_prologue(void* grad_slab, int64_t zero_slab_rows, const int32_t* tile_cost, int32_t* tile_order,
                               int ntx, int tile_row0, int nt, hipStream_t s) {
    const int grid = render_grid(nt);
    const bool ordered = tile_cost != nullptr && nt >= GS_LPT_MIN_TILES;
    const size_t n_floats = (size_t)zero_slab_rows * 9;
    if (tile_order == nullptr && n_floats == 0) return GS_OK;
    const size_t want = (n_floats / 4 + 1023) / 1024;
    const int fill_blocks =
        n_floats == 0 ? 0 : (int)(want < (size_t)GS_PROLOGUE_FILL_BLOCKS ? (want ? want : 1) : GS_PROLOGUE_FILL_BLOCKS);
    k_bwd_prologue<<<(tile_order != nullptr ? 1 : 0) + fill_blocks, 1024, 0, s>>>(
        tile_cost, tile_row0 * ntx, nt, grid, tile_order, ordered ? 1 : 0, (float*)grad_slab, n_floats);
    return GS_OK;
}

int gs_render_backward_prologue(void* grad_slab, int64_t zero_slab_rows, const int32_t* tile_cost, int32_t* tile_order,
                                int W, int H, int tile_row0, int tile_row1, void* stream) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    GS_REQUIRE(tile_cost == nullptr || tile_order != nullptr, "tile_cost needs tile_order");
    GS_REQUIRE(zero_slab_rows >= 0 && (zero_slab_rows == 0 || (grad_slab != nullptr && ((uintptr_t)grad_slab & 15) == 0)),
               "zero_slab_rows must be >= 0 and the slab 16-byte aligned");
    if (int e = check_rows(H, tile_row0, tile_row1)) return e;
    const int ntx = (W + 15) / 16;
    if (int e = launch_bwd_prologue(grad_slab, zero_slab_rows, tile_cost, tile_order, ntx, tile_row0,
                                    (tile_row1 - tile_row0) * ntx, (hipStream_t)stream))
        return e;
    return check_launch("render_backward_prologue");
}

extern "C++" {   // (a template cannot have C linkage)
// gs_render_tiles_backward_slab_m and gs_render_tiles_backward_slab_abs: one argument check, one prologue, one pair of
// launches; ABS picks the kernel (k_render_bwd<float, 1> with its recorded argument layout, or k_render_bwd_abs).
template <bool ABS>
static int launch_bwd_slab(const char* name, const void* packed, const void* rgb, const int32_t* tile_ranges,
                           const int32_t* sorted_gaussians, const void* background_rgb,
                           const int32_t* num_splats_per_pixel,
                           const void* final_weight_per_pixel, const void* grad_image, int W,
                           int H, int tile_row0, int tile_row1, void* grad_slab, int64_t zero_slab_rows,
                           const int32_t* tile_cost, int32_t* tile_order, const void* segment_state,
                           const int32_t* cut_flags, const int32_t* full_ranges, const int32_t* overflow_sorted,
                           int backward_mode, const uint64_t* touch_masks, void* grad_uv_abs, void* stream) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    GS_REQUIRE(!ABS || grad_uv_abs != nullptr, "grad_uv_abs must be given");
    GS_REQUIRE(tile_cost == nullptr || tile_order != nullptr, "tile_cost needs tile_order (tile_cost and tile_order go together)");
    GS_REQUIRE((cut_flags == nullptr) == (full_ranges == nullptr) && (cut_flags == nullptr) == (overflow_sorted == nullptr),
               "cut_flags, full_ranges and overflow_sorted go together");
    GS_REQUIRE(segment_state == nullptr || ((uintptr_t)segment_state & 15) == 0, "segment_state must be 16-byte aligned");
    GS_REQUIRE(zero_slab_rows >= 0 && (zero_slab_rows == 0 || ((uintptr_t)grad_slab & 15) == 0),
               "zero_slab_rows must be >= 0 and the slab 16-byte aligned");
    if (int e = check_rows(H, tile_row0, tile_row1)) return e;
    int exact = 0;
    if (int e = resolve_backward_mode(backward_mode, &exact)) return e;
    hipStream_t s = (hipStream_t)stream;
    const int ntx = (W + 15) / 16;
    const int nt = (tile_row1 - tile_row0) * ntx;
    const int grid = render_grid(nt);
    // tile_order without tile_cost: the order gs_render_backward_prologue left there.  With tile_cost (or rows to
    // clear) the prologue runs here.
    const bool order_given = tile_cost == nullptr && tile_order != nullptr;
    const bool use_order = segment_state == nullptr && (order_given || (tile_cost != nullptr && nt >= GS_LPT_MIN_TILES));
    if (!order_given)
        if (int e = launch_bwd_prologue(grad_slab, zero_slab_rows,
                                        segment_state == nullptr && nt >= GS_LPT_MIN_TILES ? tile_cost : nullptr,
                                        use_order ? tile_order : nullptr, ntx, tile_row0, nt, s))
            return e;
    if (order_given && zero_slab_rows > 0)
        if (int e = launch_bwd_prologue(grad_slab, zero_slab_rows, nullptr, nullptr, ntx, tile_row0, nt, s)) return e;
    if (nt == 0) return check_launch(name);
    // One launch for the four cases.  With segment_state: (tile, depth segment) work items from the state the forward
    // left (gs_render_tiles_prefix / _packed with the same segment_state); segment-major launch order = most work first,
    // no order kernel (use_order is false), no LDS padding.  tail: what the kernel takes after touch_masks.
    const bool segmented = segment_state != nullptr;
    auto launch = [&](auto kernel, auto... tail) {
        kernel<<<segmented ? grid * SEG_MAX : grid, RB, segmented ? 0 : GS_BWD_LDS_PAD, s>>>(
            (const float*)packed, (const float*)rgb, nullptr, tile_ranges, sorted_gaussians,
            (const float*)background_rgb, num_splats_per_pixel, (const float*)final_weight_per_pixel,
            (const float*)grad_image, W, H, ntx, tile_row0 * ntx, nt, (float*)grad_slab, nullptr,
            nullptr, nullptr, 1, exact, use_order ? tile_order : nullptr, nullptr, nullptr,
            segmented ? seg_state_of((void*)segment_state, W, H, tile_row0, tile_row1) : SEG_NONE,
            cut_flags, full_ranges, overflow_sorted, (const unsigned long long*)touch_masks, tail...);
    };
    if constexpr (ABS) launch(k_render_bwd_abs, (float*)grad_uv_abs);
    else launch(k_render_bwd<float, 1>);
    return check_launch(name);
}

}   // extern "C++"

int gs_render_tiles_backward_slab_m(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                  const int32_t* sorted_gaussians, const void* background_rgb,
                                  const int32_t* num_splats_per_pixel,
                                  const void* final_weight_per_pixel, const void* grad_image, int W,
                                  int H, int tile_row0, int tile_row1, void* grad_slab, int64_t zero_slab_rows,
                                  const int32_t* tile_cost, int32_t* tile_order, const void* segment_state,
                                  const int32_t* cut_flags, const int32_t* full_ranges, const int32_t* overflow_sorted,
                                  int backward_mode, const uint64_t* touch_masks, void* stream) {
    return launch_bwd_slab<false>("render_tiles_backward_slab", packed, rgb, tile_ranges, sorted_gaussians, background_rgb,
                                  num_splats_per_pixel, final_weight_per_pixel, grad_image, W, H, tile_row0, tile_row1,
                                  grad_slab, zero_slab_rows, tile_cost, tile_order, segment_state, cut_flags, full_ranges,
                                  overflow_sorted, backward_mode, touch_masks, nullptr, stream);
}

int gs_render_tiles_backward_slab_abs(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                      const int32_t* sorted_gaussians, const void* background_rgb,
                                      const int32_t* num_splats_per_pixel,
                                      const void* final_weight_per_pixel, const void* grad_image, int W,
                                      int H, int tile_row0, int tile_row1, void* grad_slab, int64_t zero_slab_rows,
                                      const int32_t* tile_cost, int32_t* tile_order, const void* segment_state,
                                      const int32_t* cut_flags, const int32_t* full_ranges, const int32_t* overflow_sorted,
                                      int backward_mode, const uint64_t* touch_masks, void* grad_uv_abs, void* stream) {
    return launch_bwd_slab<true>("render_tiles_backward_slab_abs", packed, rgb, tile_ranges, sorted_gaussians, background_rgb,
                                 num_splats_per_pixel, final_weight_per_pixel, grad_image, W, H, tile_row0, tile_row1,
                                 grad_slab, zero_slab_rows, tile_cost, tile_order, segment_state, cut_flags, full_ranges,
                                 overflow_sorted, backward_mode, touch_masks, grad_uv_abs, stream);
}

int gs_render_tiles_backward_slab(const void* packed, const void* rgb, const int32_t* tile_ranges,
                                  const int32_t* sorted_gaussians, const void* background_rgb,
                                  const int32_t* num_splats_per_pixel,
                                  const void* final_weight_per_pixel, const void* grad_image, int W,
                                  int H, int tile_row0, int tile_row1, void* grad_slab, int64_t zero_slab_rows,
                                  const int32_t* tile_cost, int32_t* tile_order, const void* segment_state,
                                  const int32_t* cut_flags, const int32_t* full_ranges, const int32_t* overflow_sorted,
                                  int backward_mode, void* stream) {
    return gs_render_tiles_backward_slab_m(packed, rgb, tile_ranges, sorted_gaussians, background_rgb, num_splats_per_pixel,
                                           final_weight_per_pixel, grad_image, W, H, tile_row0, tile_row1, grad_slab, zero_slab_rows,
                                           tile_cost, tile_order, segment_state, cut_flags, full_ranges, overflow_sorted,
                                           backward_mode, nullptr, stream);
}

int gs_render_depth(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                    const int32_t* sorted_gaussians, int W, int H, float alpha_threshold,
                    void* depth_image, void* stream) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    hipStream_t s = (hipStream_t)stream;
    const int ntx = (W + 15) / 16, nty = (H + 15) / 16;
    const int nt = ntx * nty;
    const int grid = render_grid(nt);
    k_render_depth<<<grid, RB, 0, s>>>((const float*)packed, (const float*)xyz_camera_frame,
                                       tile_ranges, sorted_gaussians, W, H, ntx, nt,
                                       alpha_threshold, (float*)depth_image);
    return check_launch("render_depth");
}

// What the four map entry points (`name`) check alike, in the order each always did, and the tiles of the call's rows.
// The forward passes its three outputs (transmittance among them); the backward transmittance, an input there, and no
// map_out / alpha_out.  n_channels: 1 for the depth map.  (packed, the channel source and sorted_gaussians are only
// read where a list has entries: V == 0 passes anything)
struct MapTiles {
    int ntx, tile0, nt;   // nt == 0: nothing to launch
};
static int map_entry_tiles(const char* name, bool backward, int n_channels, const void* packed,
                           const int32_t* tile_ranges, const int32_t* num_splats_per_pixel, const void* transmittance,
                           const void* map_out, const void* alpha_out, int W, int H, int tile_row0, int tile_row1,
                           MapTiles* t) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    GS_REQUIRE(n_channels >= 1 && n_channels <= 32, "%s: n_channels must be in 1..32", name);
    if (backward) {
        GS_REQUIRE(tile_ranges != nullptr && num_splats_per_pixel != nullptr && transmittance != nullptr,
                   "%s: tile_ranges, num_splats_per_pixel or transmittance is NULL", name);
    } else {
        GS_REQUIRE(tile_ranges != nullptr && num_splats_per_pixel != nullptr,
                   "%s: tile_ranges or num_splats_per_pixel is NULL", name);
        GS_REQUIRE(map_out != nullptr && alpha_out != nullptr && transmittance != nullptr, "%s: an output is NULL",
                   name);
    }
    GS_REQUIRE(((uintptr_t)packed & 15) == 0, "%s: packed must be 16-byte aligned", name);
    if (int e = check_rows(H, tile_row0, tile_row1)) return e;
    t->ntx = (W + 15) / 16;
    t->tile0 = tile_row0 * t->ntx;
    t->nt = (tile_row1 - tile_row0) * t->ntx;
    return GS_OK;
}

int gs_render_zalpha(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                     const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel, int W, int H,
                     int tile_row0, int tile_row1, void* depth, void* alpha, void* transmittance, void* stream) {
    MapTiles t;
    if (int e = map_entry_tiles("render_zalpha", false, 1, packed, tile_ranges, num_splats_per_pixel, transmittance,
                                depth, alpha, W, H, tile_row0, tile_row1, &t))
        return e;
    if (t.nt == 0) return GS_OK;
    k_render_zalpha_fwd<<<render_grid(t.nt), RB, 0, (hipStream_t)stream>>>(
        (const float*)packed, (const float*)xyz_camera_frame, tile_ranges, sorted_gaussians, num_splats_per_pixel, W, H,
        t.ntx, t.tile0, t.nt, (float*)depth, (float*)alpha, (float*)transmittance);
    return check_launch("render_zalpha");
}

int gs_render_zalpha_backward(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                              const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel,
                              const void* transmittance, const void* grad_depth, const void* grad_alpha, int W, int H,
                              int tile_row0, int tile_row1, void* grad_slab, void* grad_z, void* stream) {
    MapTiles t;
    if (int e = map_entry_tiles("render_zalpha_backward", true, 1, packed, tile_ranges, num_splats_per_pixel,
                                transmittance, nullptr, nullptr, W, H, tile_row0, tile_row1, &t))
        return e;
    if (t.nt == 0 || (grad_depth == nullptr && grad_alpha == nullptr)) return GS_OK;   // nothing to add
    GS_REQUIRE(grad_slab != nullptr && grad_z != nullptr, "render_zalpha_backward: grad_slab or grad_z is NULL");
    k_render_zalpha_bwd<<<render_grid(t.nt), RB, 0, (hipStream_t)stream>>>(
        (const float*)packed, (const float*)xyz_camera_frame, tile_ranges, sorted_gaussians, num_splats_per_pixel,
        (const float*)transmittance, (const float*)grad_depth, (const float*)grad_alpha, W, H, t.ntx, t.tile0, t.nt,
        (float*)grad_slab, (float*)grad_z);
    return check_launch("render_zalpha_backward");
}

int gs_render_distortion(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                         const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel, int W, int H,
                         int tile_row0, int tile_row1, void* distortion, void* depth, void* alpha, void* transmittance,
                         void* stream) {
    MapTiles t;
    if (int e = map_entry_tiles("render_distortion", false, 1, packed, tile_ranges, num_splats_per_pixel, transmittance,
                                depth, alpha, W, H, tile_row0, tile_row1, &t))
        return e;
    GS_REQUIRE(distortion != nullptr, "render_distortion: an output is NULL");
    if (t.nt == 0) return GS_OK;
    k_render_distortion_fwd<<<render_grid(t.nt), RB, 0, (hipStream_t)stream>>>(
        (const float*)packed, (const float*)xyz_camera_frame, tile_ranges, sorted_gaussians, num_splats_per_pixel, W, H,
        t.ntx, t.tile0, t.nt, (float*)distortion, (float*)depth, (float*)alpha, (float*)transmittance);
    return check_launch("render_distortion");
}

int gs_render_distortion_backward(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                                  const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel,
                                  const void* transmittance, const void* depth, const void* alpha,
                                  const void* grad_distortion, const void* grad_depth, const void* grad_alpha, int W,
                                  int H, int tile_row0, int tile_row1, void* grad_slab, void* grad_z, void* stream) {
    MapTiles t;
    if (int e = map_entry_tiles("render_distortion_backward", true, 1, packed, tile_ranges, num_splats_per_pixel,
                                transmittance, nullptr, nullptr, W, H, tile_row0, tile_row1, &t))
        return e;
    GS_REQUIRE(depth != nullptr && alpha != nullptr, "render_distortion_backward: depth or alpha is NULL");
    if (t.nt == 0 || (grad_distortion == nullptr && grad_depth == nullptr && grad_alpha == nullptr))
        return GS_OK;   // nothing to add
    GS_REQUIRE(grad_slab != nullptr && grad_z != nullptr, "render_distortion_backward: grad_slab or grad_z is NULL");
    k_render_distortion_bwd<<<render_grid(t.nt), RB, 0, (hipStream_t)stream>>>(
        (const float*)packed, (const float*)xyz_camera_frame, tile_ranges, sorted_gaussians, num_splats_per_pixel,
        (const float*)transmittance, (const float*)depth, (const float*)alpha, (const float*)grad_distortion,
        (const float*)grad_depth, (const float*)grad_alpha, W, H, t.ntx, t.tile0, t.nt, (float*)grad_slab,
        (float*)grad_z);
    return check_launch("render_distortion_backward");
}

int gs_render_median_depth(const void* packed, const void* xyz_camera_frame, const int32_t* tile_ranges,
                           const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel, int W, int H,
                           int tile_row0, int tile_row1, void* median_depth, int32_t* median_index, void* depth,
                           void* alpha, void* transmittance, void* stream) {
    MapTiles t;
    if (int e = map_entry_tiles("render_median_depth", false, 1, packed, tile_ranges, num_splats_per_pixel,
                                transmittance, depth, alpha, W, H, tile_row0, tile_row1, &t))
        return e;
    GS_REQUIRE(median_depth != nullptr && median_index != nullptr, "render_median_depth: an output is NULL");
    if (t.nt == 0) return GS_OK;
    k_render_median_fwd<<<render_grid(t.nt), RB, 0, (hipStream_t)stream>>>(
        (const float*)packed, (const float*)xyz_camera_frame, tile_ranges, sorted_gaussians, num_splats_per_pixel, W, H,
        t.ntx, t.tile0, t.nt, (float*)median_depth, median_index, (float*)depth, (float*)alpha, (float*)transmittance);
    return check_launch("render_median_depth");
}

int gs_median_depth_backward(const int32_t* median_index, const void* grad_median_depth, int W, int H,
                             int tile_row0, int tile_row1, void* grad_z, void* stream) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    GS_REQUIRE(median_index != nullptr, "median_depth_backward: median_index is NULL");
    if (int e = check_rows(H, tile_row0, tile_row1)) return e;
    const int ntx = (W + 15) / 16;
    const int nt = (tile_row1 - tile_row0) * ntx;
    if (nt == 0 || grad_median_depth == nullptr) return GS_OK;   // nothing to add
    GS_REQUIRE(grad_z != nullptr, "median_depth_backward: grad_z is NULL");
    k_median_depth_bwd<<<render_grid(nt), RB, 0, (hipStream_t)stream>>>(
        median_index, (const float*)grad_median_depth, W, H, ntx, tile_row0 * ntx, nt, (float*)grad_z);
    return check_launch("median_depth_backward");
}

int gs_render_features(const void* packed, const void* features, int n_channels, const int32_t* tile_ranges,
                       const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel, int W, int H,
                       int tile_row0, int tile_row1, void* feature_map, void* alpha, void* transmittance,
                       void* stream) {
    MapTiles t;
    if (int e = map_entry_tiles("render_features", false, n_channels, packed, tile_ranges, num_splats_per_pixel,
                                transmittance, feature_map, alpha, W, H, tile_row0, tile_row1, &t))
        return e;
    if (t.nt == 0) return GS_OK;
    DISPATCH_CP(n_channels, (k_render_features_fwd<CP><<<render_grid(t.nt), RB, 0, (hipStream_t)stream>>>(
        (const float*)packed, (const float*)features, n_channels, tile_ranges, sorted_gaussians, num_splats_per_pixel,
        W, H, t.ntx, t.tile0, t.nt, (float*)feature_map, (float*)alpha, (float*)transmittance)));
    return check_launch("render_features");
}

int gs_render_features_backward(const void* packed, const void* features, int n_channels, const int32_t* tile_ranges,
                                const int32_t* sorted_gaussians, const int32_t* num_splats_per_pixel,
                                const void* transmittance, const void* grad_feature_map, const void* grad_alpha, int W,
                                int H, int tile_row0, int tile_row1, void* grad_slab, void* grad_features,
                                void* stream) {
    MapTiles t;
    if (int e = map_entry_tiles("render_features_backward", true, n_channels, packed, tile_ranges,
                                num_splats_per_pixel, transmittance, nullptr, nullptr, W, H, tile_row0, tile_row1, &t))
        return e;
    if (t.nt == 0 || (grad_feature_map == nullptr && grad_alpha == nullptr)) return GS_OK;   // nothing to add
    GS_REQUIRE(grad_slab != nullptr, "render_features_backward: grad_slab is NULL");
    DISPATCH_CP(n_channels, (k_render_features_bwd<CP><<<render_grid(t.nt), RB, 0, (hipStream_t)stream>>>(
        (const float*)packed, (const float*)features, n_channels, tile_ranges, sorted_gaussians, num_splats_per_pixel,
        (const float*)transmittance, (const float*)grad_feature_map, (const float*)grad_alpha, W, H, t.ntx, t.tile0,
        t.nt, (float*)grad_slab, (float*)grad_features)));
    return check_launch("render_features_backward");
}

// entries staged per chunk of k_render_contrib: 64 (the backward walks') or 256 (the forward walks').  Measured in
// alternating blocks of one process (profiles/r13/contributions_cost.json): 64 is 9 % faster at workload B (short
// lists: 6.3 KB of LDS and 49 VGPRs against 25.3 KB and 73) and within 0.5 % of 256 at D
#ifndef GS_CONTRIB_CHUNK
#define GS_CONTRIB_CHUNK 64
#endif
static std::atomic<int> g_contrib_chunk{GS_CONTRIB_CHUNK};

int gs_debug_contributions_chunk(int chunk) {
    const int before = g_contrib_chunk.load(std::memory_order_relaxed);
    if (chunk == 0) return before;
    GS_REQUIRE(chunk == 64 || chunk == 256, "gs_debug_contributions_chunk: 64, 256 or 0 (query)");
    g_contrib_chunk.store(chunk, std::memory_order_relaxed);
    return before;
}

int gs_render_contributions(const void* packed, const int32_t* tile_ranges, const int32_t* sorted_gaussians,
                            const int32_t* num_splats_per_pixel, const int32_t* row_index, int W, int H,
                            int tile_row0, int tile_row1, void* weight_sum, void* weight_max,
                            int32_t* pixel_count, void* stream) {
    GS_REQUIRE(W > 0 && H > 0, "image must be non-empty");
    GS_REQUIRE(tile_ranges != nullptr && num_splats_per_pixel != nullptr,
               "render_contributions: tile_ranges or num_splats_per_pixel is NULL");
    GS_REQUIRE(((uintptr_t)packed & 15) == 0, "render_contributions: packed must be 16-byte aligned");
    if (int e = check_rows(H, tile_row0, tile_row1)) return e;
    const int ntx = (W + 15) / 16;
    const int tile0 = tile_row0 * ntx, nt = (tile_row1 - tile_row0) * ntx;
    if (nt == 0 || (weight_sum == nullptr && weight_max == nullptr && pixel_count == nullptr)) return GS_OK;
    if (g_contrib_chunk.load(std::memory_order_relaxed) != 256)
        k_render_contrib<64><<<render_grid(nt), RB, 0, (hipStream_t)stream>>>(
            (const float*)packed, tile_ranges, sorted_gaussians, num_splats_per_pixel, row_index, W, H, ntx, tile0, nt,
            (float*)weight_sum, (int*)weight_max, pixel_count);
    else
        k_render_contrib<256><<<render_grid(nt), RB, 0, (hipStream_t)stream>>>(
            (const float*)packed, tile_ranges, sorted_gaussians, num_splats_per_pixel, row_index, W, H, ntx, tile0, nt,
            (float*)weight_sum, (int*)weight_max, pixel_count);
    return check_launch("render_contributions");
}

}  // extern "C"
