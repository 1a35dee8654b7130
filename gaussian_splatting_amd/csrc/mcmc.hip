// mcmc.hip -- the device side of MCMC densification ("3D Gaussian Splatting as Markov Chain Monte Carlo";
// gaussian_splatting_amd/densify.py: MCMCController).  No reference counterpart: the reference knows only the
// clone / split / delete heuristics of densify.hip.
//
//   gs_mcmc_relocate    dead Gaussians are moved onto sampled live ones IN PLACE, many destinations per source, and
//                       every Gaussian sampled n - 1 times gets the opacity and scale that leave the rendered image
//                       unchanged when n copies of it are composited (the paper's eq. 9).  The correction is an
//                       alternating binomial sum: fp32 loses up to four digits of it, so it is
//                       evaluated in double and rounded once.  It touches the sampled rows only, once per refinement
//                       step: the double arithmetic costs nothing that matters.
//   gs_mcmc_add_noise   xyz += Sigma_world (noise * gate(opacity) * step), every iteration over all N Gaussians: one
//                       pass of 68 bytes per Gaussian (56 read, 12 written).
#include "pg_math.h"

namespace gs {

constexpr int MC_MAX_TENSORS = 8;
enum { MC_PLAIN = 0, MC_SCALE = 2, MC_OPACITY = 4 };   // 0 and 2 as gs_densify_move numbers them

struct McmcTensors {
    float* p[MC_MAX_TENSORS];
    float* m[MC_MAX_TENSORS];   // exp_avg (or null: no optimizer state for this tensor yet)
    float* v[MC_MAX_TENSORS];   // exp_avg_sq
    int width[MC_MAX_TENSORS];        // floats per row
    int width_end[MC_MAX_TENSORS];    // inclusive prefix of width
    int n, opacity, scale;            // tensor count, index of the opacity and of the scale tensor
};

// The largest opacity the correction takes: 1 - 2^-24, the largest fp32 below 1.  (A logit above ~16.6 gives 1.0 in
// fp32, where 1 - o is 0 and the correction has no value.)
__device__ inline double mc_opacity_max() { return 1.0 - 5.9604644775390625e-08; }

// Opacity and log-scale offset of a Gaussian that stands for one of n equal copies of (o, scale):
//   o_new = 1 - (1 - o)^(1/n)
//   denom = sum_{k=0..n-1} C(n,k+1) (-1)^k o_new^(k+1) / sqrt(k+1)     (the hockey-stick form of the paper's double sum
//           sum_{i=1..n} sum_{k=0..i-1} C(i-1,k) (-1)^k o_new^(k+1) / sqrt(k+1))
//   scale_new = scale + log(o / denom)
// o_new is formed as -expm1(log1p(-o) / n): the same function without the cancellation of 1 - (1 - o)^(1/n) at small o.
// The binomials run C(n,k+1) = C(n,k) (n-k) / (k+1): every product stays below 2^53 for n <= 51 (the largest is
// C(51,25) * 26 = 6.4e15), so each is exact.
__device__ inline void mc_relocation(double o, int n, double* o_new_out, double* log_ratio_out) {
    const double o_new = -expm1(log1p(-o) / (double)n);
    double binom = 1.0, power = 1.0, denom = 0.0;
    for (int k = 0; k < n; k++) {
        binom = binom * (double)(n - k) / (double)(k + 1);   // C(n, k+1)
        power = power * o_new;                               // o_new^(k+1)
        const double term = binom * power / __builtin_sqrt((double)(k + 1));
        denom = (k & 1) ? denom - term : denom + term;
    }
    *o_new_out = o_new;
    *log_ratio_out = log(o / denom);
}

// launch A: one thread per row; rows with ratio <= 1 are neither read nor written
__global__ __launch_bounds__(256) void k_mcmc_correct(McmcTensors T, const int* __restrict__ ratio, int n_rows,
                                                      float min_opacity) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int times = ratio[r];
    if (times <= 1) return;
    const int n = times < GS_MCMC_MAX_RATIO ? times : GS_MCMC_MAX_RATIO;
    float* opa = T.p[T.opacity] + r;
    float* sc = T.p[T.scale] + (size_t)r * 3;
    const double o = fmin(1.0 / (1.0 + exp(-(double)*opa)), mc_opacity_max());
    double o_new, log_ratio;
    mc_relocation(o, n, &o_new, &log_ratio);
    const double oc = fmin(fmax(o_new, (double)min_opacity), mc_opacity_max());
    *opa = (float)log(oc / (1.0 - oc));
#pragma unroll
    for (int c = 0; c < 3; c++) sc[c] = (float)((double)sc[c] + log_ratio);
    for (int k = 0; k < T.n; k++) {
        if (!T.m[k]) continue;
        const size_t base = (size_t)r * T.width[k];
        for (int c = 0; c < T.width[k]; c++) {
            T.m[k][base + c] = 0.0f;
            T.v[k][base + c] = 0.0f;
        }
    }
}

// launch B: one thread per (destination, element of the concatenated row); consecutive threads copy consecutive
// floats of one source row to one destination row
__global__ __launch_bounds__(256) void k_mcmc_move(McmcTensors T, const int* __restrict__ dst_rows,
                                                   const int* __restrict__ src_rows, int M) {
    const int row_floats = T.width_end[T.n - 1];
    const long long total = (long long)M * row_floats;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(e / row_floats);
        const int at = (int)(e - (long long)m * row_floats);
        int k = 0;
        while (at >= T.width_end[k]) k++;
        const int col = at - (k ? T.width_end[k - 1] : 0);
        const size_t from = (size_t)src_rows[m] * T.width[k] + col, to = (size_t)dst_rows[m] * T.width[k] + col;
        T.p[k][to] = T.p[k][from];
        if (T.m[k]) {
            T.m[k][to] = 0.0f;
            T.v[k][to] = 0.0f;
        }
    }
}

// One thread per Gaussian.  A wave reads 64 consecutive rows of every tensor: 1 KiB of quaternions as one 16-byte load
// per lane, 768 contiguous bytes of xyz / scale / noise as 12-byte loads per lane and 256 bytes of opacity, so every
// cache line a wave touches it consumes whole in the same instruction; nothing is read twice.  All five loads are
// issued before the first use.  The exponentials are the library's det_expf (gs_common.h), as in sigma_world_of.
__global__ __launch_bounds__(256) void k_mcmc_add_noise(float* __restrict__ xyz, const float4* __restrict__ quaternion,
                                                        const float* __restrict__ scale,
                                                        const float* __restrict__ opacity,
                                                        const float* __restrict__ noise, int N, float step,
                                                        float gate_k, float gate_x0) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const size_t i3 = (size_t)i * 3;
    const float4 qv = quaternion[i];
    const float s3[3] = {scale[i3], scale[i3 + 1], scale[i3 + 2]};
    const float e3[3] = {noise[i3], noise[i3 + 1], noise[i3 + 2]};
    const float x3[3] = {xyz[i3], xyz[i3 + 1], xyz[i3 + 2]};
    const float logit = opacity[i];
    const float q4[4] = {qv.x, qv.y, qv.z, qv.w};
    const float o = 1.0f / (1.0f + det_expf(-logit));
    const float gate = 1.0f / (1.0f + det_expf(-gate_k * ((1.0f - o) - gate_x0)));
    float S[9];
    sigma_world_of<float>(q4, s3, S);
    const float f = gate * step;
    const float e0 = e3[0] * f, e1 = e3[1] * f, e2 = e3[2] * f;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float d = (S[3 * r] * e0 + S[3 * r + 1] * e1) + S[3 * r + 2] * e2;
        xyz[i3 + r] = x3[r] + d;
    }
}

}  // namespace gs

using namespace gs;

extern "C" int gs_mcmc_relocate(int n_tensors, void* const* params, void* const* exp_avg, void* const* exp_avg_sq,
                                const int32_t* width, const int32_t* kind, int n_rows, const int32_t* ratio,
                                const int32_t* dst_rows, const int32_t* src_rows, int M, float min_opacity,
                                void* stream) {
    GS_REQUIRE(n_tensors >= 1 && n_tensors <= MC_MAX_TENSORS, "gs_mcmc_relocate takes 1..%d tensors", MC_MAX_TENSORS);
    GS_REQUIRE(n_rows >= 0 && M >= 0, "mcmc_relocate: bad sizes");
    McmcTensors T;
    int n_opacity = 0, n_scale = 0, end = 0;
    T.opacity = T.scale = 0;
    for (int k = 0; k < n_tensors; k++) {
        GS_REQUIRE(width[k] > 0 && (kind[k] == MC_PLAIN || kind[k] == MC_SCALE || kind[k] == MC_OPACITY),
                   "mcmc_relocate: bad width / kind for tensor %d", k);
        GS_REQUIRE(kind[k] != MC_SCALE || width[k] == 3, "mcmc_relocate: scale rows have 3 floats");
        GS_REQUIRE(kind[k] != MC_OPACITY || width[k] == 1, "mcmc_relocate: opacity rows have 1 float");
        GS_REQUIRE(params[k] != nullptr, "mcmc_relocate: tensor %d is NULL", k);
        GS_REQUIRE((exp_avg[k] == nullptr) == (exp_avg_sq[k] == nullptr),
                   "mcmc_relocate: exp_avg and exp_avg_sq go together");
        if (kind[k] == MC_OPACITY) { T.opacity = k; n_opacity++; }
        if (kind[k] == MC_SCALE) { T.scale = k; n_scale++; }
        T.p[k] = (float*)params[k];
        T.m[k] = (float*)exp_avg[k];
        T.v[k] = (float*)exp_avg_sq[k];
        T.width[k] = width[k];
        end += width[k];
        T.width_end[k] = end;
    }
    GS_REQUIRE(n_opacity == 1 && n_scale == 1,
               "mcmc_relocate needs exactly one opacity tensor (kind 4) and one scale tensor (kind 2): got %d and %d",
               n_opacity, n_scale);
    for (int k = n_tensors; k < MC_MAX_TENSORS; k++) {
        T.p[k] = T.m[k] = T.v[k] = nullptr;
        T.width[k] = 0;
        T.width_end[k] = end;
    }
    T.n = n_tensors;
    if (M == 0 || n_rows == 0) return GS_OK;
    GS_REQUIRE(ratio != nullptr && dst_rows != nullptr && src_rows != nullptr,
               "mcmc_relocate: ratio / dst_rows / src_rows is NULL with M > 0");
    k_mcmc_correct<<<div_up(n_rows, 256), 256, 0, (hipStream_t)stream>>>(T, ratio, n_rows, min_opacity);
    const int status = check_launch("mcmc_relocate (correction)");
    if (status != GS_OK) return status;
    const long long blocks = ((long long)M * end + 255) / 256;
    k_mcmc_move<<<(int)(blocks < 4096 ? blocks : 4096), 256, 0, (hipStream_t)stream>>>(T, dst_rows, src_rows, M);
    return check_launch("mcmc_relocate (move)");
}

extern "C" int gs_mcmc_add_noise(void* xyz, const void* quaternion, const void* scale, const void* opacity,
                                 const void* noise, int N, float step, float gate_k, float gate_x0, void* stream) {
    GS_REQUIRE(N >= 0, "mcmc_add_noise: N < 0");
    if (N == 0) return GS_OK;
    GS_REQUIRE(xyz && quaternion && scale && opacity && noise, "mcmc_add_noise: NULL tensor with N > 0");
    GS_REQUIRE(((uintptr_t)quaternion & 15) == 0, "mcmc_add_noise: quaternion must be 16-byte aligned");
    k_mcmc_add_noise<<<div_up(N, 256), 256, 0, (hipStream_t)stream>>>(
        (float*)xyz, (const float4*)quaternion, (const float*)scale, (const float*)opacity, (const float*)noise, N, step,
        gate_k, gate_x0);
    return check_launch("mcmc_add_noise");
}
