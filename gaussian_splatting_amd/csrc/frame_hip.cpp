// frame_hip.cpp -- native orchestration of one fused frame: the Python module `gsplat_frame`.
//
// gaussian_splatting_amd/fused.py in C++: the same two autograd nodes (per-Gaussian stage + binning +
// sort | render), the same C-ABI calls in the same order on torch's current HIP stream, the same single
// 8-byte host read per frame with the speculative emit / sort / render enqueued before it -- but the
// frame costs one Python call and the backward runs inside the C++ autograd engine, so that a 0.5 ms
// frame (workload B, or one band of a multi-GPU frame) is no longer bound by ~0.5 ms of interpreter
// time.  Contract of rasterize(): splat_py.rasterize.rasterize (reference:
// splat_py/rasterize.py:18-112) -> (image, culling_mask, uv); `uv` is an output of the first node and an
// input of the second, so uv.retain_grad() / uv.grad work as the trainer expects (trainer.py:360,379).
// fp32, SH-precompute colour mode (what fused.supported() accepts); everything else stays on the
// reference-shaped path.
#include <ATen/hip/HIPContext.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>
#include <torch/extension.h>
#include <torch/csrc/distributed/c10d/ProcessGroup.hpp>
#include <torch/csrc/jit/python/python_ivalue.h>

#include <cstdlib>
#include <map>
#include <string>
#include <mutex>
#include <tuple>
#include <vector>

#include "../../include/gsplat_hip.h"
#include "frame_policy.h"

namespace {

using torch::Tensor;
using torch::autograd::AutogradContext;
using torch::autograd::variable_list;

void ok(int status) { TORCH_CHECK(status == GS_OK, gs_last_error()); }
void hip_ok(hipError_t e) { TORCH_CHECK(e == hipSuccess, "HIP: ", hipGetErrorString(e)); }
void* cur_stream() { return (void*)c10::hip::getCurrentHIPStream().stream(); }

constexpr int SLAB_WIDTH = 9;   // rgb 3 | opacity 1 | uv 2 | conic 3

// ---- per-process state: one record per frame shape, pinned read buffers, counters -------------------------------
using namespace frame_policy;
static_assert(PREFIX_RENDER == GS_PREFIX_RENDER && PREFIX_REPAIR == GS_PREFIX_REPAIR, "frame_policy.h vs gsplat_hip.h");
struct HintKey {
    int dev, N, T, row0, row1;
    bool operator<(const HintKey& o) const {
        return std::tie(dev, N, T, row0, row1) < std::tie(o.dev, o.N, o.T, o.row0, o.row1);
    }
};
// frame_policy.h's record of a shape + the pinned int32[1] the repair kernel of its cut frames writes (undefined until
// the shape's first cut frame)
struct ShapeRecord : ShapeState {
    Tensor cut_flagged;
};
std::mutex g_mutex;
std::map<HintKey, ShapeRecord> g_shapes;
struct PinnedRing {
    std::vector<Tensor> bufs;
    std::vector<hipEvent_t> events;
    size_t next = 0;
};
std::map<int, PinnedRing> g_pinned;   // per device
struct Counters {
    int64_t frames = 0, speculative = 0, misses = 0, s_min = -1, s_max = -1, slab_copies = 0, cut_frames = 0, cut_backoffs = 0;
    int64_t render_only = 0, late_repairs = 0, long_list_misses = 0;   // the longest-list guess of complete-list frames
} g_counters;
std::vector<Tensor> g_flag_log;
Tensor g_last_flags;   // tile_flags of the latest prefix-mode render (tests / tools)
// tests / tools (fused.keep_last_slab): a reference to the [V, 9] slab of the latest per-Gaussian backward
bool g_keep_slab = false;
Tensor g_last_slab;
// (also bound for the Python orchestration: with this module loaded there is ONE slot, whichever path ran last)
void note_slab(Tensor slab) {
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_keep_slab) g_last_slab = std::move(slab);
}
Policy g_policy;
bool g_band_compact = true;   // multi-GPU: band-compact per-Gaussian stage (OwnerPreprocess)
// band-compact frames: the fused frontend (gs_band_frontend, ABI 8) and the gathering per-Gaussian backward; false =
// the three-call pipeline of rounds 3-5 (gs_band_project, gs_halo_plan_masked, gs_preprocess_forward_list;
// gs_halo_gather_sum), kept for A/B measurements and as the checker of the fused form (tests/test_gpu_band_frontend.py)
bool g_band_fused = true;
// the render backward reads the touch masks its forward built (512 bytes per tile) instead of rebuilding them
bool g_touch_masks = true;
// the histogram gs_preprocess_forward_cut fills and returns to zero: one per (device, stream), zeroed once
int32_t* depth_hist_of(const torch::Device& dev, void* stream) {
    static std::map<std::pair<int, void*>, Tensor> hists;
    std::lock_guard<std::mutex> lock(g_mutex);
    auto key = std::make_pair((int)dev.index(), stream);
    auto it = hists.find(key);
    if (it == hists.end())
        it = hists.emplace(key, torch::zeros({GS_CUT_HIST_BINS}, torch::TensorOptions().dtype(torch::kInt32).device(dev))).first;
    return it->second.data_ptr<int32_t>();
}

// optional per-entry-point timing (bench.py): events on the launch stream around every C-ABI call, so the
// elapsed time of one entry point is the GPU time of the kernels it enqueues
struct Timing {
    bool on = false;
    std::string only;   // non-empty: only this entry point is timed
    std::map<std::string, std::vector<std::pair<hipEvent_t, hipEvent_t>>> spans;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        hip_ok(hipEventCreate(&e));
        return e;
    }
} g_timing;

template <typename F> void timed(const char* name, void* stream, F&& call) {
    if (!g_timing.on || (!g_timing.only.empty() && g_timing.only != name)) {
        ok(call());
        return;
    }
    hipEvent_t a, b;
    {
        std::lock_guard<std::mutex> lock(g_mutex);
        a = g_timing.get();
        b = g_timing.get();
    }
    hip_ok(hipEventRecord(a, (hipStream_t)stream));
    ok(call());
    hip_ok(hipEventRecord(b, (hipStream_t)stream));
    std::lock_guard<std::mutex> lock(g_mutex);
    g_timing.spans[name].push_back({a, b});
}

// one float 0 per device (a stride-0 stand-in for gradients nobody reads: no fill kernel per frame)
Tensor zero_scalar(const torch::Device& dev) {
    static std::map<int, Tensor> zeros;
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = zeros.find((int)dev.index());
    if (it == zeros.end())
        it = zeros.emplace((int)dev.index(), torch::zeros({1}, torch::TensorOptions().dtype(torch::kFloat32).device(dev))).first;
    return it->second;
}

std::pair<int32_t*, hipEvent_t> pinned_slot(int dev) {
    PinnedRing& ring = g_pinned[dev];
    if (ring.bufs.empty()) {
        for (int i = 0; i < 4; i++) {
            ring.bufs.push_back(torch::empty({96}, torch::TensorOptions().dtype(torch::kInt32).pinned_memory(true)));
            hipEvent_t ev;
            hip_ok(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            ring.events.push_back(ev);
        }
    }
    ring.next = (ring.next + 1) % ring.bufs.size();
    return {ring.bufs[ring.next].data_ptr<int32_t>(), ring.events[ring.next]};
}

// ---- the two critical sections of a frame --------------------------------------------------------------------
// At its start a frame decides on the depth cut, takes a copy of its shape's record -- every guess of the frame comes
// from that copy -- and the pinned slot of its host read.  may_cut: a whole single-GPU frame.
struct FrameStart {
    ShapeState st;
    bool cut = false;
    int32_t* cut_word = nullptr;   // cut frames: where the render's repair kernel leaves its flagged-tile count
    int32_t* host = nullptr;
    hipEvent_t ready = nullptr;
};
FrameStart begin_frame(const HintKey& shape, int ntx, bool may_cut, int sort_prefix) {
    FrameStart s;
    std::lock_guard<std::mutex> lock(g_mutex);
    ShapeRecord& rec = g_shapes[shape];
    if (may_cut) {
        volatile int32_t* w = rec.cut_flagged.defined() ? rec.cut_flagged.data_ptr<int32_t>() : nullptr;
        const CutDecision d =
            want_depth_cut(rec, g_policy, shape.N, (int64_t)(shape.row1 - shape.row0) * ntx, true, sort_prefix, w ? *w : 0,
                           [&](int n) { return gs_cut_supported(ntx, shape.row0, shape.row1, n) != 0; });
        if (d.clear_word) *w = 0;
        g_counters.cut_backoffs += d.backoff;
        if ((s.cut = d.cut)) {
            if (!w) rec.cut_flagged = torch::zeros({1}, torch::TensorOptions().dtype(torch::kInt32).pinned_memory(true));
            s.cut_word = rec.cut_flagged.data_ptr<int32_t>();
        }
    }
    s.st = rec;
    std::tie(s.host, s.ready) = pinned_slot(shape.dev);
    return s;
}
// After its host read a frame counts itself and leaves what it learned in the (live) record.  V >= 0: the frame also
// reports the complete and the visible count the "auto" cut decides on (single-GPU frames).  -> does the exact render
// of this frame (o.act == Act::Render, complete lists) take the depth-segmented backward
bool finish_frame(const HintKey& shape, const FrameKind& k, const FramePlan& f, const FrameOutcome& o, const FrameCounts& c,
                  int64_t n_tiles, int64_t V = -1) {
    std::lock_guard<std::mutex> lock(g_mutex);
    g_counters.frames++;
    g_counters.speculative += f.speculative;
    g_counters.cut_frames += k.cut;
    g_counters.s_min = g_counters.s_min < 0 ? c.S_complete : std::min(g_counters.s_min, c.S_complete);
    g_counters.s_max = std::max(g_counters.s_max, c.S_complete);
    g_counters.misses += o.miss;
    g_counters.long_list_misses += o.unsorted_long;
    g_counters.late_repairs += o.act == Act::LateRepair;
    g_counters.render_only += o.render_only;
    ShapeRecord& rec = g_shapes[shape];
    learn(rec, k, c);
    if (V >= 0) {
        rec.complete_count = c.S_complete;
        rec.visible_count = V;
    }
    return o.act == Act::Render && !k.cut && segments_for(rec, g_policy, c.S, true, n_tiles);
}

// one allocation cut into 1-D blocks, each starting 16-byte aligned
struct Arena {
    Tensor buf;
    std::vector<int64_t> offsets;
    Arena(c10::ScalarType dtype, c10::Device dev, std::initializer_list<int64_t> sizes) {
        int64_t off = 0;
        for (int64_t n : sizes) {
            offsets.push_back(off);
            off += (n + 3) & ~int64_t(3);
        }
        buf = torch::empty({off}, torch::TensorOptions().dtype(dtype).device(dev));
    }
    template <typename T> T* ptr(size_t i) { return buf.data_ptr<T>() + offsets[i]; }
    Tensor block(size_t i, int64_t n) { return buf.narrow(0, offsets[i], n); }
};

// the gradients of one per-Gaussian backward over n Gaussians: xyz | quaternion | scale | opacity | rgb | sh in one
// allocation, handed to autograd as views (the first six inputs of both first nodes)
struct ParamGrads {
    int64_t n, n_sh;
    Arena a;
    ParamGrads(c10::Device dev, int64_t n, int n_sh)
        : n(n), n_sh(n_sh), a(torch::kFloat32, dev, {3 * n, 4 * n, 3 * n, n, 3 * n, 3 * (int64_t)(n_sh - 1) * n}) {}
    float* ptr(size_t i) { return i == 5 && n_sh <= 1 ? nullptr : a.ptr<float>(i); }
    void views(variable_list& out) {
        static const int64_t widths[5] = {3, 4, 3, 1, 3};
        for (int k = 0; k < 5; k++) out[k] = a.block(k, widths[k] * n).view({n, widths[k]});
        if (n_sh > 1) out[5] = a.block(5, 3 * (n_sh - 1) * n).view({n, 3, n_sh - 1});
    }
};

void require_f32_cuda(const Tensor& t, const char* name, c10::Device dev, std::initializer_list<int64_t> shape) {
    TORCH_CHECK(t.is_cuda() && t.device() == dev, name, " is not a CUDA tensor on ", dev);
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " is not a float tensor");
    bool same = t.dim() == (int64_t)shape.size();
    int64_t d = 0;
    for (int64_t s : shape) same = same && t.size(d++) == s;
    TORCH_CHECK(same, name, " has the wrong shape ", t.sizes());
}
// what every frame entry point demands of its tensors before their pointers go to the C ABI; -> an sh tensor is given
bool check_frame_inputs(const Tensor& xyz, const Tensor& quaternion, const Tensor& scale, const Tensor& opacity,
                        const Tensor& rgb, const c10::optional<Tensor>& sh, const Tensor& camera_T_world, const Tensor& K,
                        const Tensor& background_rgb, int64_t width, int64_t height) {
    const auto dev = xyz.device();
    const int64_t N = xyz.size(0);
    TORCH_CHECK(xyz.is_cuda(), "xyz is not a CUDA tensor");
    require_f32_cuda(xyz, "xyz", dev, {N, 3});
    require_f32_cuda(quaternion, "quaternion", dev, {N, 4});
    require_f32_cuda(scale, "scale", dev, {N, 3});
    require_f32_cuda(opacity, "opacity", dev, {N, 1});
    require_f32_cuda(rgb, "rgb", dev, {N, 3});
    require_f32_cuda(camera_T_world, "camera_T_world", dev, {4, 4});
    require_f32_cuda(K, "K", dev, {3, 3});
    require_f32_cuda(background_rgb, "background_rgb", dev, {3});
    const bool has_sh = sh.has_value() && sh->defined();
    if (has_sh) {
        TORCH_CHECK(sh->is_cuda() && sh->device() == dev, "sh is not a CUDA tensor on ", dev);
        TORCH_CHECK(sh->scalar_type() == torch::kFloat32, "sh is not a float tensor");
        TORCH_CHECK(sh->dim() == 3 && sh->size(0) == N && sh->size(1) == 3 &&
                        (sh->size(2) == 3 || sh->size(2) == 8 || sh->size(2) == 15),
                    "sh has the wrong shape ", sh->sizes());
    }
    TORCH_CHECK(width > 0 && height > 0, "image must be non-empty");
    return has_sh;
}

struct RenderOut {
    Tensor buf, image, fw, nsp, seg;   // seg: state for the depth-segmented backward (empty: not segmented)
    Tensor cut_flags, overflow_sorted;   // depth-cut frames: flagged tiles and their complete lists (else undefined)
    Tensor prefix_flags;                 // prefix-sorted frames: the provisional render's tile flags (else undefined)
    int32_t* tile_cost = nullptr;        // per-tile render cost int32[T] inside buf (the backward's launch-order key)
    Tensor masks;                        // touch masks the forward left for the backward (include/gsplat_hip.h, `_m` entries)
};
// what gs_render_tiles_cut needs from the frame's binning
struct CutRef {
    const float* bin_rec;
    int32_t *tile_counts, *cut_ws, *full_ranges;
    int N;
    float mh;
    int64_t overflow_capacity;
    int32_t* host_flagged;
};

// The prefix render of a frame, in phases, on the buffers in r.  GS_PREFIX_REPAIR alone: the repair phase of a frame
// whose render was enqueued without it (the guess "no list exceeds the prefix" turned out wrong): full sort + second
// render of the flagged tiles
void render_prefix(RenderOut& r, const float* packed, const float* rgbr, const int32_t* ranges, Tensor& sorted, Tensor& keys,
                   const Tensor& bg, int W, int H, int row0, int row1, int phases, void* stream) {
    timed("gs_render_tiles_prefix", stream, [&] {
        return gs_render_tiles_prefix_phased_m(packed, rgbr, ranges, sorted.data_ptr<int32_t>(),
                                               (const uint64_t*)keys.data_ptr<int64_t>(), sorted.size(0), bg.data_ptr(), W, H, row0,
                                               row1, r.prefix_flags.data_ptr<int32_t>(), r.nsp.data_ptr<int32_t>(),
                                               r.fw.data_ptr(), r.image.data_ptr(), r.tile_cost,
                                               r.seg.numel() > 0 ? r.seg.data_ptr() : nullptr, phases,
                                               r.masks.defined() ? (uint64_t*)r.masks.data_ptr<int64_t>() : nullptr, stream);
    });
}

RenderOut render_forward(const float* packed, const float* rgbr, const int32_t* ranges, Tensor& sorted, Tensor& keys,
                         const Tensor& bg, int W, int H, int row0, int row1, bool whole, int sort_prefix, void* stream,
                         bool segments, int64_t image_rows = 0, const CutRef* cut = nullptr,
                         int prefix_phases = GS_PREFIX_RENDER | GS_PREFIX_REPAIR) {
    const int64_t P = (int64_t)W * H;
    // image_rows > H (multi-GPU, equal bands): the image block holds world_size full bands so that the band
    // images can be all-gathered in place; the kernels only see the first H rows
    const int64_t PI = std::max<int64_t>(image_rows, H) * W;
    auto opt = torch::TensorOptions().dtype(torch::kFloat32).device(bg.device());
    RenderOut r;
    // one allocation: image [H,W,3] | final weight [H,W] | splat count [H,W] (int32 view) | per-tile render
    // cost int32[T] | launch-order workspace int32[T + 8] (the backward finds the last two behind the splat
    // counts: tile_cost_of()).  Rows outside [row0, row1) are not written by the kernel: zero-fill only when
    // restricted
    const int ntx = (W + 15) / 16, nty = (H + 15) / 16;
    const int64_t T = (int64_t)ntx * nty;
    r.buf = whole ? torch::empty({3 * PI + 2 * P + 2 * T + 8}, opt) : torch::zeros({3 * PI + 2 * P + 2 * T + 8}, opt);
    r.image = r.buf.narrow(0, 0, 3 * PI).view({-1, W, 3});
    r.fw = r.buf.narrow(0, 3 * PI, P).view({H, W});
    r.nsp = r.buf.narrow(0, 3 * PI + P, P).view(torch::kInt32).view({H, W});
    int32_t* tile_cost = r.tile_cost = reinterpret_cast<int32_t*>(r.buf.data_ptr<float>()) + 3 * PI + 2 * P;
    // the prefix / cut render leaves touch masks for the backward; its tile flags go to the log of tests and tools
    auto touch_masks = [&] {
        if (g_touch_masks) r.masks = torch::empty({T * 64}, opt.dtype(torch::kInt64));
    };
    auto log_flags = [&](const Tensor& flags) {
        std::lock_guard<std::mutex> lock(g_mutex);
        if (g_flag_log.size() < 512) g_flag_log.push_back(flags);
        g_last_flags = flags;
    };
    if (cut != nullptr) {
        // depth-cut lists: kept prefixes, then (on the device, only if a tile was flagged) the complete lists of the
        // flagged tiles from the overflow buffers
        r.seg = torch::empty({0}, opt);
        r.cut_flags = torch::empty({T}, opt.dtype(torch::kInt32));
        // (never empty: a frame without a visible Gaussian still hands the backward a non-null overflow list)
        const int64_t ocap = std::max<int64_t>(cut->overflow_capacity, 1);
        r.overflow_sorted = torch::empty({ocap}, opt.dtype(torch::kInt32));
        Tensor okeys = torch::empty({ocap}, opt.dtype(torch::kInt64));
        touch_masks();
        uint64_t* masks_p = r.masks.defined() ? (uint64_t*)r.masks.data_ptr<int64_t>() : nullptr;
        timed("gs_render_tiles_prefix", stream, [&] {
            return gs_render_tiles_cut_m(packed, rgbr, ranges, sorted.data_ptr<int32_t>(), sorted.size(0), cut->full_ranges,
                                         cut->bin_rec, cut->N, cut->mh, cut->tile_counts, cut->cut_ws,
                                         (uint64_t*)okeys.data_ptr<int64_t>(), r.overflow_sorted.data_ptr<int32_t>(),
                                         cut->overflow_capacity, bg.data_ptr(), W, H, row0, row1,
                                         r.cut_flags.data_ptr<int32_t>(), r.nsp.data_ptr<int32_t>(), r.fw.data_ptr(),
                                         r.image.data_ptr(), tile_cost, cut->host_flagged, masks_p, stream);
        });
        log_flags(r.cut_flags);
        return r;
    }
    r.seg = torch::empty({segments ? (int64_t)(gs_render_segment_workspace_bytes(W, H, row0, row1) / 4) : 0}, opt);
    if (sort_prefix && sorted.size(0) > sort_prefix) {
        r.prefix_flags = torch::empty({(int64_t)ntx * nty}, opt.dtype(torch::kInt32));
        touch_masks();
        render_prefix(r, packed, rgbr, ranges, sorted, keys, bg, W, H, row0, row1, prefix_phases, stream);
        log_flags(r.prefix_flags);
    } else {
        void* seg_p = segments ? r.seg.data_ptr() : nullptr;
        // no costs measured: all tiles equal (any launch order is as good as another)
        TORCH_CHECK(hipMemsetAsync(tile_cost, 0, sizeof(int32_t) * (size_t)T, (hipStream_t)stream) == hipSuccess,
                    "hipMemsetAsync failed");
        timed("gs_render_tiles_packed", stream, [&] {
            return gs_render_tiles_packed(packed, rgbr, nullptr, ranges, sorted.data_ptr<int32_t>(), bg.data_ptr(), W, H, 1, row0, row1,
                                   r.nsp.data_ptr<int32_t>(), r.fw.data_ptr(), r.image.data_ptr(), GS_F32, seg_p, stream);
        });
    }
    return r;
}

// ---- the opt-in fused optimizer step (train_ops.FusedRasterAdam) --------------------------------------------
// The plan is a Python object kept alive by the graph; Preprocess::backward calls its begin() -- at backward time,
// under the GIL, after the node has unpacked its saved tensors -- and gets what gs_preprocess_backward_adam takes:
//   ([(param, exp_avg, exp_avg_sq, lr, step) for quaternion, scale, opacity, rgb, sh (None without SH)], beta1, beta2, eps)
using PlanHolder = c10::intrusive_ptr<c10::ivalue::PyObjectHolder>;
struct AdamRows {
    Tensor p[5], m[5], v[5];
    double lr[5] = {0, 0, 0, 0, 0};
    int64_t step[5] = {1, 1, 1, 1, 1};
    double beta1 = 0, beta2 = 0, eps = 0;
};
AdamRows adam_begin(PyObject* plan) {
    AdamRows a;
    std::string error;
    {
        py::gil_scoped_acquire gil;
        try {
            py::tuple t = py::reinterpret_borrow<py::object>(plan).attr("begin")();
            py::sequence rows = t[0];
            TORCH_CHECK(py::len(rows) == 5, "the optimizer plan must describe five tensors");
            for (int k = 0; k < 5; k++) {
                if (py::object(rows[k]).is_none()) continue;
                py::tuple r = rows[k];
                a.p[k] = r[0].cast<Tensor>();
                a.m[k] = r[1].cast<Tensor>();
                a.v[k] = r[2].cast<Tensor>();
                a.lr[k] = r[3].cast<double>();
                a.step[k] = r[4].cast<int64_t>();
            }
            a.beta1 = t[1].cast<double>();
            a.beta2 = t[2].cast<double>();
            a.eps = t[3].cast<double>();
        } catch (py::error_already_set& e) {
            error = e.what();   // (the Python error is released under the GIL, here)
        }
    }
    TORCH_CHECK(error.empty(), error);
    return a;
}

// ---- node 1: parameters -> uv, conic, opacity, colour (+ the frame's lists and, early, its image) --------
// its outputs: the four differentiable per-splat tensors, then what node 2 and the caller take over
enum PreOutput {
    PRE_UV, PRE_CONIC, PRE_OPACITY, PRE_RGB, PRE_PACKED, PRE_RANGES, PRE_SORTED, PRE_MASK, PRE_IMAGE, PRE_FW, PRE_NSP,
    PRE_SEG, PRE_CUT_FLAGS, PRE_FULL_RANGES, PRE_OVERFLOW, PRE_MASKS, PRE_OUTPUTS
};
struct Preprocess : public torch::autograd::Function<Preprocess> {
    static variable_list forward(AutogradContext* ctx, Tensor xyz, Tensor quaternion, Tensor scale, Tensor opacity,
                                 Tensor rgb, c10::optional<Tensor> sh_opt, Tensor camera_T_world, Tensor K, Tensor bg,
                                 int64_t W, int64_t H, double near_thresh, double far_thresh, double padding,
                                 double mh_dist, int64_t row0, int64_t row1, PlanHolder adam_plan, int64_t raster_mode,
                                 c10::optional<Tensor> filter3d_opt) {
        // filter3d: the 3D smoothing filter's variances [N] (a constant: no edge), or nothing -- the _filtered entries with
        // NULL launch what the _mode entries launch
        // raster_mode: the bit mask of include/gsplat_hip.h.  GS_RASTER_ANTIALIASED: the record's opacity carries
        // sqrt(det Sigma_2D / det(Sigma_2D + 0.25 I)); GS_RASTER_FISHEYE: uv, the cull and the projection Jacobian are the
        // equidistant fisheye model's.  Only the per-Gaussian kernels differ, forward and backward -- binning, sort and
        // render are the classic frame's
        const auto dev = xyz.device();
        const int N = (int)xyz.size(0);
        const bool has_sh = sh_opt.has_value() && sh_opt->defined();
        Tensor sh = has_sh ? sh_opt->contiguous() : Tensor();
        const int n_sh = has_sh ? (int)sh.size(2) + 1 : 1;
        const bool has_filter = filter3d_opt.has_value() && filter3d_opt->defined();
        Tensor filter3d = has_filter ? filter3d_opt->contiguous() : Tensor();
        const int ntx = ((int)W + 15) / 16, nty = ((int)H + 15) / 16, T = ntx * nty;
        const bool whole = row0 == 0 && row1 == nty;
        const int sort_prefix = g_policy.sort_prefix ? GS_SORT_PREFIX : 0;
        void* stream = cur_stream();

        const HintKey shape{(int)dev.index(), N, T, (int)row0, (int)row1};
        const FrameStart start = begin_frame(shape, ntx, whole, sort_prefix);
        const bool cut = start.cut;
        int32_t* const host = start.host;
        const int stride = cut ? gs_cut_sample_stride(N) : 1;
        const int64_t n_ws = (int64_t)gs_preprocess_workspace_ints(N), n_tc = (int64_t)gs_tile_workspace_ints(T);
        const int64_t n_cut = cut ? (int64_t)gs_cut_workspace_ints(N, T) : 0;
        // int blocks: workspace | V | rank | vis_idx | tile workspace | ranges (+ S', V, S) | mask bytes | cut workspace |
        // complete ranges;  float blocks: centre | uv | xyz_cam | conic | opacity | colour | packed | binning records.
        // With the depth cut, uv / conic / z live in the 32-byte binning records (columns 0-1, 2-4, 5) and the separate
        // arrays are not written: the tensors this node hands on are strided views of the records.
        const int64_t nn = N;
        Arena iar(torch::kInt32, dev, {n_ws, 1, N, 0, n_tc, T + 3, (N + 3) / 4, n_cut, cut ? T + 1 : 0});
        Arena far(torch::kFloat32, dev, {3, cut ? 0 : 2 * nn, cut ? 0 : 3 * nn, cut ? 0 : 3 * nn, N, 0, 12 * nn,
                                         cut ? 8 * nn : 0});
        int32_t *ws = iar.ptr<int32_t>(0), *count = iar.ptr<int32_t>(1), *rank = iar.ptr<int32_t>(2),
                *tile_counts = iar.ptr<int32_t>(4), *ranges_buf = iar.ptr<int32_t>(5);
        uint8_t* mask = (uint8_t*)iar.ptr<int32_t>(6);
        int32_t *cut_ws = iar.ptr<int32_t>(7), *full_ranges = iar.ptr<int32_t>(8);
        float *center = far.ptr<float>(0), *uv = far.ptr<float>(1), *xyz_cam = far.ptr<float>(2), *conic = far.ptr<float>(3),
              *opa = far.ptr<float>(4), *packed = far.ptr<float>(6), *bin_rec = far.ptr<float>(7);
        // (the one-coefficient render kernels read the colour from the packed record: no separate colour array)
        const float* rgbr = packed;
        int32_t* depth_hist = cut ? depth_hist_of(dev, stream) : nullptr;
        timed("gs_preprocess_forward", stream, [&] {
            return gs_preprocess_forward_filtered(
                xyz.data_ptr(), quaternion.data_ptr(), scale.data_ptr(), opacity.data_ptr(), rgb.data_ptr(),
                has_sh ? sh.data_ptr() : nullptr, n_sh, camera_T_world.data_ptr(), K.data_ptr(), N, (int)W, (int)H,
                (float)near_thresh, (float)far_thresh, (float)padding, (float)mh_dist, (int)row0, (int)row1, ws, center,
                count, mask, rank, nullptr /* vis_idx: nobody reads it on this path */, cut ? nullptr : uv,
                cut ? nullptr : xyz_cam, cut ? nullptr : conic, opa,
                nullptr /* rgb_render: the colour is in the packed record */, packed, cut ? bin_rec : nullptr,
                cut ? cut_ws : nullptr, depth_hist, stride, has_filter ? filter3d.data_ptr() : nullptr, (int)raster_mode,
                stream);
        });
        const FrameKind kind{cut, sort_prefix, !cut && sort_prefix != 0, true};
        const FramePlan plan = plan_frame(start.st, g_policy, kind);
        timed("gs_tile_count", stream, [&] {
            if (cut)
                return gs_tile_count_cut(bin_rec, N, count, ntx, nty, (float)mh_dist, (int)row0, (int)row1, tile_counts, cut_ws,
                                         ranges_buf, full_ranges, host, stream);
            return gs_tile_count(uv, conic, N, count, nullptr, nullptr, ntx, nty, (float)mh_dist, (int)row0, (int)row1,
                                 tile_counts, ranges_buf, host, stream);
        });
        // (the scan kernel of the count wrote the frame's counts into the pinned slot: no copy in the stream)
        hip_ok(hipEventRecord(start.ready, (hipStream_t)stream));

        auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(dev);
        Tensor sorted, keys;
        auto emit_sort = [&](int64_t capacity, int64_t longest) {
            sorted = torch::empty({capacity}, i32);
            keys = torch::empty({capacity}, i32.dtype(torch::kInt64));
            if (capacity > 0)
                timed("gs_tile_emit_sort", stream, [&] {
                    if (cut)
                        return gs_tile_emit_sort_cut(bin_rec, N, ntx, nty, (float)mh_dist, (int)row0, (int)row1, ranges_buf,
                                                     tile_counts, cut_ws, (uint64_t*)keys.data_ptr<int64_t>(), capacity,
                                                     sorted.data_ptr<int32_t>(), stream);
                    return gs_tile_emit_sort_bounded(uv, xyz_cam, conic, N, count, nullptr, nullptr, ntx, nty, (float)mh_dist,
                                                     (int)row0, (int)row1, ranges_buf, tile_counts,
                                                     (uint64_t*)keys.data_ptr<int64_t>(), capacity,
                                                     sorted.data_ptr<int32_t>(), sort_prefix, longest, stream);
                });
        };
        CutRef cref{bin_rec, tile_counts, cut_ws, full_ranges, N, (float)mh_dist, plan.overflow_capacity, start.cut_word};
        auto render = [&](Tensor& lists, Tensor& list_keys, bool segments, int phases) {
            return render_forward(packed, rgbr, ranges_buf, lists, list_keys, bg, (int)W, (int)H, (int)row0, (int)row1, whole,
                                  sort_prefix, stream, segments, 0, cut ? &cref : nullptr, phases);
        };
        RenderOut out;
        const int64_t n_tiles = (int64_t)(row1 - row0) * ntx;
        if (plan.speculative) emit_sort(plan.capacity, plan.longest_guess);
        if (plan.early_render) {
            ShapeState st = start.st;   // (a capacity is no exact count: nothing is stored)
            out = render(sorted, keys, !cut && segments_for(st, g_policy, plan.capacity, false, n_tiles), plan.phases);
        }
        // the frame's only device->host read: (S, V, longest list) -- with the depth cut (S' kept, V, S complete) --, to
        // size the outputs
        hip_ok(hipEventSynchronize(start.ready));
        const int64_t V = host[1];
        const FrameCounts counts{host[0], cut ? host[2] : host[0], cut ? -1 : host[2]};
        const int64_t S = counts.S;
        const FrameOutcome res = classify_frame(plan, kind, counts);
        const bool segments = finish_frame(shape, kind, plan, res, counts, n_tiles, V);
        if (res.re_emit) {
            cref.overflow_capacity = counts.S_complete;
            emit_sort(S, counts.longest);
        }
        Tensor sorted_g = sorted.narrow(0, 0, S), keys_g = keys.narrow(0, 0, S);
        if (res.act == Act::Render)
            out = render(sorted_g, keys_g, segments, res.phases);
        else if (res.act == Act::LateRepair)
            render_prefix(out, packed, rgbr, ranges_buf, sorted, keys, bg, (int)W, (int)H, (int)row0, (int)row1, GS_PREFIX_REPAIR,
                          stream);

        Tensor rec = cut ? far.block(7, 8 * nn).view({N, 8}).narrow(0, 0, V) : Tensor();
        variable_list o(PRE_OUTPUTS);
        o[PRE_UV] = cut ? rec.narrow(1, 0, 2) : far.block(1, 2 * nn).view({N, 2}).narrow(0, 0, V);
        o[PRE_CONIC] = cut ? rec.narrow(1, 2, 3) : far.block(3, 3 * nn).view({N, 3}).narrow(0, 0, V);
        o[PRE_OPACITY] = far.block(4, N).view({N, 1}).narrow(0, 0, V);
        // the colour output of this node only carries the autograd edge of the render gradients' colour columns (the
        // kernels read the colour from the packed record, nobody reads this tensor's values): a stride-0 placeholder
        o[PRE_RGB] = zero_scalar(dev).expand({V, 3});
        o[PRE_PACKED] = far.block(6, 12 * nn).view({N, 12});
        o[PRE_RANGES] = iar.block(5, T + 1);
        o[PRE_SORTED] = sorted_g;
        o[PRE_MASK] = iar.block(6, (N + 3) / 4).view(torch::kBool).narrow(0, 0, N);
        o[PRE_IMAGE] = out.image;
        o[PRE_FW] = out.fw;
        o[PRE_NSP] = out.nsp;
        o[PRE_SEG] = out.seg;
        // depth-cut frames: what the backward needs to read a repaired tile's complete list (empty otherwise)
        o[PRE_CUT_FLAGS] = cut ? out.cut_flags : torch::empty({0}, i32);
        o[PRE_FULL_RANGES] = cut ? iar.block(8, T + 1) : torch::empty({0}, i32);
        o[PRE_OVERFLOW] = cut ? out.overflow_sorted : torch::empty({0}, i32);
        // the touch masks the forward left for the backward (empty: the backward builds its own)
        o[PRE_MASKS] = out.masks.defined() ? out.masks : torch::empty({0}, i32.dtype(torch::kInt64));
        ctx->save_for_backward({xyz, quaternion, scale, camera_T_world, K, far.block(0, 3), iar.block(2, N),
                                far.block(4, N).view({N, 1})});
        ctx->saved_data["n_sh"] = (int64_t)n_sh;
        ctx->saved_data["V"] = V;
        if (adam_plan) ctx->saved_data["adam_plan"] = c10::IValue(adam_plan);
        // (recorded here: the node's edge indices skip an absent sh, its backward cannot ask by argument position)
        ctx->saved_data["pose_grad"] = camera_T_world.requires_grad();
        ctx->saved_data["raster_mode"] = raster_mode;
        if (has_filter) ctx->saved_data["filter3d"] = filter3d;   // (a constant without a graph: no cycle through the node)
        ctx->set_materialize_grads(false);
        ctx->mark_non_differentiable(variable_list(o.begin() + PRE_PACKED, o.end()));
        return o;
    }

    static variable_list backward(AutogradContext* ctx, variable_list g) {
        auto saved = ctx->get_saved_variables();
        const Tensor &xyz = saved[0], &quaternion = saved[1], &scale = saved[2], &camera_T_world = saved[3], &K = saved[4],
                     &center = saved[5], &rank = saved[6], &opacity_act = saved[7];
        const int n_sh = (int)ctx->saved_data["n_sh"].toInt();
        const int64_t V = ctx->saved_data["V"].toInt();
        const int N = (int)xyz.size(0);
        const auto dev = xyz.device();
        const Tensor &g_uv = g[0], &g_conic = g[1], &g_opa = g[2], &g_rgb = g[3];
        // the four render gradients as one [V, 9] slab: the slab they are views of when they come straight
        // from Render::backward, a packed copy otherwise (outputs nobody consumed count as 0)
        Tensor slab;
        {
            auto is_col = [&](const Tensor& t, int64_t start, int64_t width, const Tensor& base) {
                return t.defined() && t.dim() == 2 && t.size(0) == V && t.size(1) == width && t.stride(0) == SLAB_WIDTH &&
                       t.stride(1) == 1 && t.is_alias_of(base) && t.storage_offset() == base.storage_offset() + start;
            };
            if (g_rgb.defined() && g_rgb._base().defined()) {
                Tensor base(g_rgb._base());
                if (base.dim() == 2 && base.size(1) == SLAB_WIDTH && base.is_contiguous() && is_col(g_rgb, 0, 3, base) &&
                    is_col(g_opa, 3, 1, base) && is_col(g_uv, 4, 2, base) && is_col(g_conic, 6, 3, base))
                    slab = base;
            }
            if (!slab.defined()) {
                {
                    std::lock_guard<std::mutex> lock(g_mutex);
                    g_counters.slab_copies++;
                }
                slab = torch::zeros({std::max<int64_t>(V, 1), SLAB_WIDTH}, xyz.options());
                if (g_rgb.defined()) slab.narrow(0, 0, V).narrow(1, 0, 3).copy_(g_rgb);
                if (g_opa.defined()) slab.narrow(0, 0, V).narrow(1, 3, 1).copy_(g_opa);
                if (g_uv.defined()) slab.narrow(0, 0, V).narrow(1, 4, 2).copy_(g_uv);
                if (g_conic.defined()) slab.narrow(0, 0, V).narrow(1, 6, 3).copy_(g_conic);
            }
        }
        const int64_t n = N, extra = 3 * (int64_t)(n_sh - 1);
        const int raster_mode = (int)ctx->saved_data["raster_mode"].toInt();
        const void* filter3d = ctx->saved_data.count("filter3d") ? ctx->saved_data["filter3d"].toTensor().data_ptr() : nullptr;
        variable_list out(20);
        if (g_keep_slab) note_slab(slab.narrow(0, 0, V));
        // camera_T_world's gradient (gs_pose_backward), before the fused optimizer step, which overwrites the quaternion
        // and scale the pose terms read
        if (ctx->saved_data["pose_grad"].toBool()) {
            void* stream = cur_stream();
            // (two allocations: the gradient outlives the backward, the workspace must not live as long)
            Tensor grad_pose = torch::empty({4, 4}, xyz.options());
            Tensor ws = torch::empty({(int64_t)gs_pose_workspace_floats(N)}, xyz.options());
            timed("gs_pose_backward", stream, [&] {
                return gs_pose_backward_filtered(xyz.data_ptr(), quaternion.data_ptr(), scale.data_ptr(),
                                                 camera_T_world.data_ptr(), K.data_ptr(), rank.data_ptr<int32_t>(),
                                                 opacity_act.data_ptr(), slab.data_ptr(), 0, N, ws.data_ptr(),
                                                 grad_pose.data_ptr(), filter3d, raster_mode, stream);
            });
            out[6] = grad_pose;
        }
        if (ctx->saved_data.count("adam_plan")) {
            // the fused optimizer step: quaternion, scale, opacity, rgb and sh are stepped by the kernel, in place;
            // only xyz gets a gradient
            AdamRows a = adam_begin(ctx->saved_data["adam_plan"].toPyObject());
            const int n_rows = n_sh > 1 ? 5 : 4;
            static const int64_t widths[5] = {4, 3, 1, 3, 0};
            for (int k = 0; k < n_rows; k++) {
                const int64_t numel = n * (k < 4 ? widths[k] : extra);
                for (const Tensor* t : {&a.p[k], &a.m[k], &a.v[k]})
                    TORCH_CHECK(t->defined() && t->is_cuda() && t->device() == dev && t->scalar_type() == torch::kFloat32 &&
                                    t->is_contiguous() && t->numel() == numel,
                                "fused optimizer step: a parameter or moment tensor has the wrong device, dtype, layout or size");
            }
            TORCH_CHECK(a.p[0].data_ptr() == quaternion.data_ptr() && a.p[1].data_ptr() == scale.data_ptr(),
                        "fused optimizer step: the plan's quaternion / scale are not the frame's");
            Tensor grad_xyz = torch::empty({n, 3}, xyz.options());
            if (n > 0) {
                void* stream = cur_stream();
                auto ptr = [](const Tensor& t) { return t.defined() ? t.data_ptr() : nullptr; };
                timed("gs_preprocess_backward_adam", stream, [&] {
                    return gs_preprocess_backward_adam(
                        xyz.data_ptr(), n_sh, camera_T_world.data_ptr(), K.data_ptr(), center.data_ptr(),
                        rank.data_ptr<int32_t>(), opacity_act.data_ptr(), slab.data_ptr(), 0, (int)n, grad_xyz.data_ptr(),
                        ptr(a.p[0]), ptr(a.m[0]), ptr(a.v[0]), a.lr[0], a.step[0], ptr(a.p[1]), ptr(a.m[1]), ptr(a.v[1]),
                        a.lr[1], a.step[1], ptr(a.p[2]), ptr(a.m[2]), ptr(a.v[2]), a.lr[2], a.step[2], ptr(a.p[3]),
                        ptr(a.m[3]), ptr(a.v[3]), a.lr[3], a.step[3], ptr(a.p[4]), ptr(a.m[4]), ptr(a.v[4]), a.lr[4],
                        a.step[4], a.beta1, a.beta2, a.eps, stream);
                });
                // the kernel wrote through raw pointers: bump the version counters like an in-place torch op would
                for (int k = 0; k < n_rows; k++)
                    for (const Tensor* t : {&a.p[k], &a.m[k], &a.v[k]}) t->unsafeGetTensorImpl()->bump_version();
            }
            out[0] = grad_xyz;
            return out;
        }
        ParamGrads ga(dev, n, n_sh);
        if (n > 0) {
            void* stream = cur_stream();
            timed("gs_preprocess_backward", stream, [&] {
                return gs_preprocess_backward_filtered(xyz.data_ptr(), quaternion.data_ptr(), scale.data_ptr(), n_sh,
                                                       camera_T_world.data_ptr(), K.data_ptr(), center.data_ptr(),
                                                       rank.data_ptr<int32_t>(), opacity_act.data_ptr(), slab.data_ptr(), 0,
                                                       (int)n, ga.ptr(0), ga.ptr(1), ga.ptr(2), ga.ptr(3), ga.ptr(4),
                                                       ga.ptr(5), filter3d, raster_mode, stream);
            });
        }
        ga.views(out);
        return out;
    }
};

// ---- node 2: the per-splat quantities + lists -> image (already enqueued by node 1) ------------------------
struct Render : public torch::autograd::Function<Render> {
    static Tensor forward(AutogradContext* ctx, Tensor uv, Tensor conic, Tensor opacity, Tensor rgbr, Tensor packed,
                          Tensor ranges, Tensor sorted_g, Tensor bg, Tensor image, Tensor fw, Tensor nsp, Tensor seg,
                          Tensor cut_flags, Tensor full_ranges, Tensor overflow_sorted, Tensor masks, int64_t row0,
                          int64_t row1) {
        ctx->save_for_backward({packed, rgbr, ranges, sorted_g, bg, nsp, fw, seg, cut_flags, full_ranges, overflow_sorted, masks});
        ctx->saved_data["row0"] = row0;
        ctx->saved_data["row1"] = row1;
        ctx->saved_data["V"] = uv.size(0);
        // this frame's gradient mode = the default at its forward (a later gs_set_backward_mode cannot race
        // the backward, which the autograd engine runs on its own thread)
        ctx->saved_data["bwd_mode"] = (int64_t)gs_get_backward_mode();
        ctx->set_materialize_grads(false);
        return image;
    }

    static variable_list backward(AutogradContext* ctx, variable_list g) {
        variable_list out(18);
        if (!g[0].defined()) return out;
        auto s = ctx->get_saved_variables();
        const Tensor &packed = s[0], &rgbr = s[1], &ranges = s[2], &sorted_g = s[3], &bg = s[4], &nsp = s[5], &fw = s[6],
                     &seg = s[7], &cut_flags = s[8], &full_ranges = s[9], &overflow_sorted = s[10], &masks = s[11];
        const bool cut = cut_flags.numel() > 0;
        const int64_t V = ctx->saved_data["V"].toInt();
        const int H = (int)nsp.size(0), W = (int)nsp.size(1);
        Tensor grad_image = g[0].contiguous();
        // (cleared by the backward call itself, in the launch that also orders the tiles: zero_slab_rows)
        Tensor slab = torch::empty({std::max<int64_t>(V, 1), SLAB_WIDTH}, packed.options());
        void* stream = cur_stream();
        const int row0 = (int)ctx->saved_data["row0"].toInt(), row1 = (int)ctx->saved_data["row1"].toInt();
        // the forward's per-tile costs and the order workspace sit behind the splat counts (render_forward)
        const int64_t T = (int64_t)((W + 15) / 16) * ((H + 15) / 16);
        int32_t* tile_cost = nsp.data_ptr<int32_t>() + (int64_t)W * H;
        // longest-first only pays where a workgroup lives long enough for the kernel's tail to matter: lists of a
        // few hundred entries per tile (workload B, 52 per tile: the order kernel's 6 us are not won back)
        const bool segmented = seg.numel() > 0;
        const bool ordered = !segmented && sorted_g.size(0) >= 256 * T;
        // one prologue launch (clear the slab + order the tiles), then the render kernel alone in its entry
        timed("gs_render_backward_prologue", stream, [&] {
            return gs_render_backward_prologue(slab.data_ptr(), slab.size(0), ordered ? tile_cost : nullptr,
                                               ordered ? tile_cost + T : nullptr, W, H, row0, row1, stream);
        });
        timed("gs_render_tiles_backward_slab", stream, [&] {
            return gs_render_tiles_backward_slab_m(packed.data_ptr(), rgbr.data_ptr(), ranges.data_ptr<int32_t>(),
                                                   sorted_g.data_ptr<int32_t>(), bg.data_ptr(), nsp.data_ptr<int32_t>(),
                                                   fw.data_ptr(), grad_image.data_ptr(), W, H, row0, row1, slab.data_ptr(),
                                                   0, nullptr, ordered ? tile_cost + T : nullptr,
                                                   segmented ? seg.data_ptr() : nullptr,
                                                   cut ? cut_flags.data_ptr<int32_t>() : nullptr,
                                                   cut ? full_ranges.data_ptr<int32_t>() : nullptr,
                                                   cut ? overflow_sorted.data_ptr<int32_t>() : nullptr,
                                                   (int)ctx->saved_data["bwd_mode"].toInt(),
                                                   masks.numel() > 0 ? (const uint64_t*)masks.data_ptr<int64_t>() : nullptr,
                                                   stream);
        });
        Tensor rows = slab.narrow(0, 0, V);
        out[0] = rows.narrow(1, 4, 2);   // uv
        out[1] = rows.narrow(1, 6, 3);   // conic
        out[2] = rows.narrow(1, 3, 1);   // opacity
        out[3] = rows.narrow(1, 0, 3);   // colour
        return out;
    }
};

std::tuple<Tensor, Tensor, Tensor> rasterize_impl(Tensor xyz, Tensor quaternion, Tensor scale, Tensor opacity, Tensor rgb,
                                                  c10::optional<Tensor> sh, Tensor camera_T_world, Tensor K, int64_t width,
                                                  int64_t height, double near_thresh, double far_thresh,
                                                  double cull_mask_padding, double mh_dist, Tensor background_rgb,
                                                  int64_t row0, int64_t row1, PlanHolder adam_plan,
                                                  int64_t raster_mode = GS_RASTER_CLASSIC,
                                                  c10::optional<Tensor> filter3d = c10::nullopt) {
    const bool filtered = filter3d.has_value() && filter3d->defined();
    const bool antialiased = (raster_mode & GS_RASTER_ANTIALIASED) != 0, fisheye = (raster_mode & GS_RASTER_FISHEYE) != 0;
    TORCH_CHECK((raster_mode & ~(int64_t)(GS_RASTER_ANTIALIASED | GS_RASTER_FISHEYE)) == 0,
                "raster_mode must be a combination of GS_RASTER_ANTIALIASED and GS_RASTER_FISHEYE, got ", raster_mode);
    TORCH_CHECK(!(antialiased && adam_plan), "antialiased frames do not take the fused optimizer step");
    TORCH_CHECK(!(fisheye && adam_plan), "fisheye frames do not take the fused optimizer step");
    TORCH_CHECK(!(filtered && adam_plan), "filter3d frames do not take the fused optimizer step");
    if (filtered) {
        TORCH_CHECK(filter3d->is_cuda() && filter3d->device() == xyz.device() && filter3d->scalar_type() == torch::kFloat32 &&
                        filter3d->dim() == 1 && filter3d->size(0) == xyz.size(0),
                    "filter3d must be float32 [N] on the Gaussians' device, one variance per Gaussian");
        TORCH_CHECK(!filter3d->requires_grad(), "filter3d is a constant of the frame and must not require a gradient");
    }
    check_frame_inputs(xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, background_rgb, width, height);
    const auto dev = xyz.device();
    const int64_t nty = (height + 15) / 16;
    if (row1 < 0) row1 = nty;
    TORCH_CHECK(0 <= row0 && row0 <= row1 && row1 <= nty, "bad tile row range");
    TORCH_CHECK(!antialiased || (row0 == 0 && row1 == nty), "antialiased frames are whole frames (no tile-row band)");
    TORCH_CHECK(!fisheye || (row0 == 0 && row1 == nty), "fisheye frames are whole frames (no tile-row band)");
    TORCH_CHECK(!filtered || (row0 == 0 && row1 == nty), "filter3d frames are whole frames (no tile-row band)");
    c10::DeviceGuard guard(dev);
    auto o = Preprocess::apply(xyz.contiguous(), quaternion.contiguous(), scale.contiguous(), opacity.contiguous(),
                               rgb.contiguous(), sh, camera_T_world.contiguous(), K.contiguous(), background_rgb.contiguous(),
                               width, height, near_thresh, far_thresh, cull_mask_padding, mh_dist, row0, row1, adam_plan,
                               raster_mode, filter3d);
    Tensor image = Render::apply(o[PRE_UV], o[PRE_CONIC], o[PRE_OPACITY], o[PRE_RGB], o[PRE_PACKED], o[PRE_RANGES],
                                 o[PRE_SORTED], background_rgb.contiguous(), o[PRE_IMAGE], o[PRE_FW], o[PRE_NSP], o[PRE_SEG],
                                 o[PRE_CUT_FLAGS], o[PRE_FULL_RANGES], o[PRE_OVERFLOW], o[PRE_MASKS], row0, row1);
    return std::make_tuple(image, o[PRE_MASK], o[PRE_UV]);
}

std::tuple<Tensor, Tensor, Tensor> rasterize(Tensor xyz, Tensor quaternion, Tensor scale, Tensor opacity, Tensor rgb,
                                             c10::optional<Tensor> sh, Tensor camera_T_world, Tensor K, int64_t width,
                                             int64_t height, double near_thresh, double far_thresh, double cull_mask_padding,
                                             double mh_dist, Tensor background_rgb, int64_t row0, int64_t row1,
                                             int64_t raster_mode, c10::optional<Tensor> filter3d) {
    return rasterize_impl(xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, width, height, near_thresh, far_thresh,
                          cull_mask_padding, mh_dist, background_rgb, row0, row1, PlanHolder(), raster_mode, filter3d);
}

// the same frame with the optimizer step of quaternion, scale, opacity, rgb and sh inside its backward
// (train_ops.FusedRasterAdam.rasterize): whole frames; the five tensors must be contiguous (they are updated in place)
std::tuple<Tensor, Tensor, Tensor> rasterize_adam(Tensor xyz, Tensor quaternion, Tensor scale, Tensor opacity, Tensor rgb,
                                                  c10::optional<Tensor> sh, Tensor camera_T_world, Tensor K, int64_t width,
                                                  int64_t height, double near_thresh, double far_thresh,
                                                  double cull_mask_padding, double mh_dist, Tensor background_rgb,
                                                  py::object plan) {
    TORCH_CHECK(!plan.is_none(), "rasterize_adam needs an optimizer plan");
    TORCH_CHECK(quaternion.is_contiguous() && scale.is_contiguous() && opacity.is_contiguous() && rgb.is_contiguous() &&
                    (!sh.has_value() || !sh->defined() || sh->is_contiguous()),
                "rasterize_adam: the parameters are stepped in place and must be contiguous");
    return rasterize_impl(xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, width, height, near_thresh, far_thresh,
                          cull_mask_padding, mh_dist, background_rgb, 0, -1, c10::ivalue::ConcretePyObjectHolder::create(plan));
}


// ---------------------------------------------------------------------------------------------------------
// multi-GPU: the tile-row sharded frame with owner-sliced gradients (gaussian_splatting_amd/sharded.py:
// _OwnerPreprocess / _OwnerRender, band policy "equal"), natively.  One rank's frame is ~0.4 ms of kernels at 8
// ranks; its Python orchestration cost 0.7 ms of host time per frame (profiles/r02/host_profile_world8.txt).
//   node 1   per-Gaussian stage for all N (replicated; SH colour only where the candidate window reaches the band)
//            -> gs_halo_plan (who sends which render-gradient rows to whom; its send list is the subset the
//            band's binning walks) -> binning + sort of the band, render of the band enqueued before the frame's one
//            host read (S, V + the plan's split sizes)            -> uv, culling mask
//   node 2   uv -> image: all-gather of the band images (in place, equal bands) through c10d (RCCL)
//   backward node 2: render backward over the band (depth-segmented when the band is small) -> rows of the send
//            list -> ONE all_to_all with the plan's splits -> gs_halo_gather_sum: the complete rows of the
//            Gaussians this rank owns; node 1: per-Gaussian backward of the owned slice.
// The record shared by the two nodes lives behind a one-byte "guard" tensor whose deleter frees it.
struct ShardSpec {
    int G = 1, rank = 0;
    std::vector<int32_t> bounds, owner_blocks;          // G + 1 each
    c10::intrusive_ptr<c10d::ProcessGroup> pg;          // null with the test hook
    py::object a2a_hook;                                // tests: stands in for all_to_all_single, no image gather
    int64_t band_pixel_rows = 0, padded_height = 0;
    // band layout: equal bands are all-gathered in place; any other split (cost-balanced bands) as chunks of
    // chunk_rows = 16 x tallest band + 1 pixel rows whose last row carries the band's per-row costs
    bool equal_bands = true;
    int64_t chunk_rows = 0;
    ~ShardSpec() {   // the record may die on an autograd thread: Python references are dropped under the GIL
        if (!a2a_hook.ptr()) return;
        if (Py_IsInitialized()) {
            py::gil_scoped_acquire gil;
            a2a_hook = py::object();
        } else {
            a2a_hook.release();   // interpreter already gone: nothing to release the reference into
        }
    }
};
// the numbers of a frame's exchange plan (what last_plan() reports of the latest sharded frame)
struct PlanNumbers {
    int64_t v_lo = 0, v_hi = 0, V = 0, S = 0, L = 0;
    std::vector<int64_t> send_splits, recv_splits;
    bool compact = false;
};
struct FrameRec : PlanNumbers {
    ShardSpec spec;
    Tensor xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, bg;   // the replicated values
    int N = 0, n_sh = 1, W = 0, H = 0, row0 = 0, row1 = 0, i0 = 0, i1 = 0;
    double near_thresh = 0, far_thresh = 0, padding = 0, mh_dist = 0;
    Tensor ibuf, fbuf, hbuf;   // arenas (kept alive: everything below points into them)
    Tensor packed, rgbr, ranges, sorted_g, center, rank_t, opa_act, halo_mask, halo_send, halo_ws;
    RenderOut out;
    bool fused = false;   // compact through gs_band_frontend (its workspace layout in halo_ws)
    Tensor owned_rows, rendered_uv_grad;
    // band-compact frames: the received rows and their per-sender offsets, handed from the render node's backward to
    // the per-Gaussian backward, which sums them on the spot (gs_preprocess_backward_gathered) unless somebody needs
    // the owned rows as a tensor (uv.grad retained, a loss term on uv)
    Tensor recv_rows;
    std::vector<int32_t> recv_offsets;
    bool gather_pending = false;
    // the uv output (weak: the record must not keep its own graph alive), to see whether its gradient is retained
    c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl> uv_weak{
        c10::intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl>()};
    int bwd_mode = GS_BACKWARD_COMPAT;
};
using FramePtr = std::shared_ptr<FrameRec>;
Tensor make_guard(const FramePtr& fr) {
    auto* holder = new FramePtr(fr);
    return torch::from_blob(holder, {1}, [](void* p) { delete reinterpret_cast<FramePtr*>(p); }, torch::kUInt8);
}
FrameRec& frame_of(const Tensor& guard) { return **reinterpret_cast<FramePtr*>(guard.data_ptr()); }

// cost-balanced bands: the latest frame's gathered per-row costs (pinned host memory) and the event behind the kernel
// that wrote them
struct RowCosts {
    Tensor host;
    hipEvent_t event = nullptr;
};
std::map<int, RowCosts> g_row_costs;   // per device (one slot per process let a second device's frame overwrite the first's)

struct PlanInfo : PlanNumbers {
    // tests (debug_keep_band_lists): the band's tile ranges and sorted list of the latest sharded frame, and the send
    // list that maps a band-compact row back to its visible index
    Tensor ranges, sorted_g, send_list;
} g_last_plan;
bool g_keep_band_lists = false;

template <typename F> void timed_region(const char* name, void* stream, F&& call) {
    timed(name, stream, [&] {
        call();
        return (int)GS_OK;
    });
}

struct OwnerPreprocess : public torch::autograd::Function<OwnerPreprocess> {
    static variable_list forward(AutogradContext* ctx, Tensor o_xyz, Tensor o_quaternion, Tensor o_scale, Tensor o_opacity,
                                 Tensor o_rgb, c10::optional<Tensor> o_sh, Tensor guard) {
        FrameRec& fr = frame_of(guard);
        const ShardSpec& sp = fr.spec;
        const auto dev = fr.xyz.device();
        const int N = fr.N, G = sp.G, me = sp.rank;
        const bool has_sh = fr.sh.defined();
        const int n_sh = fr.n_sh, W = fr.W, H = fr.H;
        const int ntx = (W + 15) / 16, nty = (H + 15) / 16, T = ntx * nty;
        const int row0 = fr.row0, row1 = fr.row1;
        const int sort_prefix = g_policy.sort_prefix ? GS_SORT_PREFIX : 0;
        const int plan_ints = 4 + 2 * G;
        // band-compact per-Gaussian stage (csrc/preprocess.hip): the full evaluation only for the Gaussians that can
        // reach the band, arrays compacted to those rows (row index l); everything downstream then works on rows l
        const bool compact = g_band_compact && G > 1;
        const bool fused = compact && g_band_fused;
        fr.compact = compact;
        fr.fused = fused;
        void* stream = cur_stream();

        const int64_t n_ws = (int64_t)gs_preprocess_workspace_ints(N), n_tc = (int64_t)gs_tile_workspace_ints(T);
        Arena iar(torch::kInt32, dev, {n_ws, 1, N, N, n_tc, T + 2 + plan_ints, (N + 3) / 4});
        // float blocks: centre | uv (by visible index) | xyz_cam | conic | opacity_act (by visible index) | colour |
        // packed | uv of the compact rows (compact mode; xyz_cam, conic, packed are then by compact row as well)
        Arena far(torch::kFloat32, dev, {4, 2 * (int64_t)N, 3 * (int64_t)N, 3 * (int64_t)N, N, compact ? 0 : 3 * (int64_t)N,
                                         12 * (int64_t)N, compact ? 2 * (int64_t)N : 0});
        int32_t *ws = iar.ptr<int32_t>(0), *count = iar.ptr<int32_t>(1), *rank = iar.ptr<int32_t>(2),
                *vis_idx = iar.ptr<int32_t>(3), *tile_counts = iar.ptr<int32_t>(4), *ranges_buf = iar.ptr<int32_t>(5);
        uint8_t* mask = (uint8_t*)iar.ptr<int32_t>(6);
        float *center = far.ptr<float>(0), *uv = far.ptr<float>(1), *xyz_cam = far.ptr<float>(2), *conic = far.ptr<float>(3),
              *opa = far.ptr<float>(4), *rgbr = far.ptr<float>(5), *packed = far.ptr<float>(6), *uv_l = far.ptr<float>(7);
        const int64_t n_hw = fused ? (int64_t)gs_band_frontend_workspace_ints(N, G) : (int64_t)gs_halo_workspace_ints(N, G);
        Tensor hbuf = torch::empty({2 * (int64_t)N + n_hw}, torch::TensorOptions().dtype(torch::kInt32).device(dev));
        int32_t* h = hbuf.data_ptr<int32_t>();
        int32_t* record = ranges_buf + T + 2;
        // what the binning walks: the first *items_n rows of (bin_uv, bin_conic, bin_xyz) or an index list into them
        const float *bin_uv = uv, *bin_conic = conic, *bin_xyz = xyz_cam;
        const int32_t *items_n = count, *subset = nullptr, *subset_n = nullptr;
        // the frame's host read: (S, V, -) from the tile scan and the plan record behind it.  Band-compact path: both
        // kernels write straight into the pinned slot (no copy kernel in the stream); otherwise one copy of the record
        // (a band shares the record of the single-GPU frame of its shape; it never takes the depth cut)
        const HintKey key{(int)dev.index(), N, T, row0, row1};
        const FrameStart start = begin_frame(key, ntx, false, sort_prefix);
        int32_t* const host = start.host;
        const int rec_at = compact ? 3 : 2;   // where the plan record starts in the host buffer
        if (fused) {
            // the fused band frontend: cull + band masks, scan, compaction of the API arrays and of the band's rows,
            // evaluation of the band's rows, the exchange plan (device + pinned host) -- four launches
            // h: list_g[N] | send_index[N] | frontend workspace
            timed("gs_band_frontend", stream, [&] {
                return gs_band_frontend(fr.xyz.data_ptr(), fr.quaternion.data_ptr(), fr.scale.data_ptr(), fr.opacity.data_ptr(),
                                        fr.rgb.data_ptr(), has_sh ? fr.sh.data_ptr() : nullptr, n_sh, fr.camera_T_world.data_ptr(),
                                        fr.K.data_ptr(), N, W, H, (float)fr.near_thresh, (float)fr.far_thresh, (float)fr.padding,
                                        (float)fr.mh_dist, sp.bounds.data(), sp.owner_blocks.data(), G, me, h + 2 * (int64_t)N,
                                        center, mask, rank, uv, opa, h + N, h, uv_l, xyz_cam, conic, packed, record,
                                        host + rec_at, stream);
            });
        } else if (compact) {
            timed("gs_band_project", stream, [&] {
                return gs_band_project(fr.xyz.data_ptr(), fr.scale.data_ptr(), fr.opacity.data_ptr(), fr.camera_T_world.data_ptr(),
                                       fr.K.data_ptr(), N, W, H, (float)fr.near_thresh, (float)fr.far_thresh, (float)fr.padding,
                                       (float)fr.mh_dist, sp.bounds.data(), G, ws, center, count, mask, rank, vis_idx, uv, opa,
                                       (uint32_t*)h, h + 2 * (int64_t)N, stream);
            });
            timed("gs_halo_plan", stream, [&] {
                return gs_halo_plan_masked((const uint32_t*)h, N, count, ws, sp.owner_blocks.data(), G, me, h + 2 * (int64_t)N,
                                           h + N, record, host + rec_at, stream);
            });
            timed("gs_preprocess_forward", stream, [&] {
                return gs_preprocess_forward_list(fr.xyz.data_ptr(), fr.quaternion.data_ptr(), fr.scale.data_ptr(),
                                                  fr.rgb.data_ptr(), has_sh ? fr.sh.data_ptr() : nullptr, n_sh,
                                                  fr.camera_T_world.data_ptr(), fr.K.data_ptr(), center, h + N, record, N, vis_idx,
                                                  uv, opa, uv_l, xyz_cam, conic, packed, stream);
            });
        } else {
            timed("gs_preprocess_forward", stream, [&] {
                return gs_preprocess_forward_mode(
                    fr.xyz.data_ptr(), fr.quaternion.data_ptr(), fr.scale.data_ptr(), fr.opacity.data_ptr(), fr.rgb.data_ptr(),
                    has_sh ? fr.sh.data_ptr() : nullptr, n_sh, fr.camera_T_world.data_ptr(), fr.K.data_ptr(), N, W, H,
                    (float)fr.near_thresh, (float)fr.far_thresh, (float)fr.padding, (float)fr.mh_dist, row0, row1, ws, center,
                    count, mask, rank, vis_idx, uv, xyz_cam, conic, opa, rgbr, packed, nullptr, nullptr, nullptr, 0,
                    GS_RASTER_CLASSIC /* band frames have no other mode */, stream);
            });
            // the exchange plan; its record rides on the frame's one host read, its send list is the binning's subset
            timed("gs_halo_plan", stream, [&] {
                return gs_halo_plan(uv, conic, N, count, ws, ntx, nty, (float)fr.mh_dist, sp.bounds.data(),
                                    sp.owner_blocks.data(), G, me, (uint32_t*)h, h + 2 * (int64_t)N, h + N, record, stream);
            });
            subset = G > 1 ? h + N : nullptr;
            subset_n = G > 1 ? record : nullptr;
        }
        if (compact) {
            bin_uv = uv_l;
            items_n = record;   // record[0] = rows of the send list = rows of the compact arrays
            rgbr = packed;      // (the one-coefficient render reads the colour from the record)
        }
        timed("gs_tile_count", stream, [&] {
            return gs_tile_count(bin_uv, bin_conic, N, items_n, subset, subset_n, ntx, nty, (float)fr.mh_dist, row0, row1,
                                 tile_counts, ranges_buf, compact ? host : nullptr, stream);
        });
        auto i32 = torch::TensorOptions().dtype(torch::kInt32).device(dev);
        Tensor sorted, keys;
        auto emit_sort = [&](int64_t capacity, int64_t longest) {
            sorted = torch::empty({capacity}, i32);
            keys = torch::empty({capacity}, i32.dtype(torch::kInt64));
            if (capacity > 0)
                timed("gs_tile_emit_sort", stream, [&] {
                    return gs_tile_emit_sort_bounded(bin_uv, bin_xyz, bin_conic, N, items_n, subset, subset_n, ntx, nty,
                                                     (float)fr.mh_dist, row0, row1, ranges_buf, tile_counts,
                                                     (uint64_t*)keys.data_ptr<int64_t>(), capacity,
                                                     sorted.data_ptr<int32_t>(), sort_prefix, longest, stream);
                });
        };
        // (compact frames also guess the band's LONGEST list: the tile scan reports it with the counts.  No late repair:
        // a guess that was too small repeats emit + sort + render, as a capacity miss does)
        const FrameKind kind{false, sort_prefix, compact && sort_prefix != 0, false};
        const FramePlan plan = plan_frame(start.st, g_policy, kind);
        if (!compact)
            hip_ok(hipMemcpyAsync(host, ranges_buf + T, (2 + plan_ints) * sizeof(int32_t), hipMemcpyDeviceToHost,
                                  (hipStream_t)stream));
        hip_ok(hipEventRecord(start.ready, (hipStream_t)stream));
        // a band.  With the real exchange the other bands' rows are overwritten by the all-gather and nothing reads
        // the other rows' splat counts / weights: no zero fill (5 us per frame); a stand-in exchange (tests, the
        // one-GPU measurement of a rank's frame) returns the band image with zeros outside it
        const bool whole = sp.a2a_hook.is_none();
        const int64_t image_rows =
            !sp.a2a_hook.is_none() ? 0 : (sp.equal_bands ? sp.padded_height : 16 * (int64_t)nty + sp.chunk_rows);
        const int64_t n_tiles = (int64_t)(row1 - row0) * ntx;
        auto render = [&](Tensor& lists, Tensor& list_keys, bool segments) {
            return render_forward(packed, rgbr, ranges_buf, lists, list_keys, fr.bg, W, H, row0, row1, whole, sort_prefix, stream,
                                  segments, image_rows);
        };
        if (plan.speculative) emit_sort(plan.capacity, plan.longest_guess);
        if (plan.early_render) {
            ShapeState st = start.st;   // (a capacity is no exact count: nothing is stored)
            fr.out = render(sorted, keys, segments_for(st, g_policy, plan.capacity, false, n_tiles));
        }
        hip_ok(hipEventSynchronize(start.ready));
        // the plan's host half: rows to send, V, v_lo, v_hi, send[G], recv[G]
        const int32_t* rec = host + rec_at;
        const int64_t S = host[0], V = rec[1], L = compact ? rec[0] : rec[1];
        const FrameCounts counts{S, S, compact ? host[2] : -1};   // (k_scan_tiles' host mirror: S, V, longest list)
        const FrameOutcome res = classify_frame(plan, kind, counts);
        const bool segments = finish_frame(key, kind, plan, res, counts, n_tiles);
        if (res.re_emit) emit_sort(S, counts.longest);
        Tensor sorted_g = sorted.narrow(0, 0, S), keys_g = keys.narrow(0, 0, S);
        if (res.act == Act::Render) fr.out = render(sorted_g, keys_g, segments);
        fr.v_lo = rec[2];
        fr.v_hi = rec[3];
        fr.send_splits.assign(rec + 4, rec + 4 + G);
        fr.recv_splits.assign(rec + 4 + G, rec + 4 + 2 * G);
        fr.V = V;
        fr.L = L;   // rows of the per-splat arrays the render works on (and of its gradient slab)
        fr.S = S;
        fr.ibuf = iar.buf;
        fr.fbuf = far.buf;
        fr.hbuf = hbuf;
        fr.packed = far.block(6, 12 * (int64_t)N).view({N, 12});
        fr.rgbr = compact ? fr.packed : far.block(5, 3 * (int64_t)N).view({N, 3}).narrow(0, 0, V);
        fr.ranges = iar.block(5, T + 1);
        fr.sorted_g = sorted_g;
        fr.center = far.block(0, 3);
        fr.rank_t = iar.block(2, N);
        fr.opa_act = far.block(4, N).view({N, 1});
        fr.halo_mask = hbuf.narrow(0, 0, N);
        fr.halo_send = hbuf.narrow(0, N, N);
        fr.halo_ws = hbuf.narrow(0, 2 * (int64_t)N, n_hw);
        fr.bwd_mode = gs_get_backward_mode();
        {
            std::lock_guard<std::mutex> lock(g_mutex);
            static_cast<PlanNumbers&>(g_last_plan) = fr;
            if (g_keep_band_lists) {
                int64_t n_send = 0;
                for (int64_t c : fr.send_splits) n_send += c;
                g_last_plan.ranges = fr.ranges.clone();
                g_last_plan.sorted_g = fr.sorted_g.clone();
                g_last_plan.send_list = fr.halo_send.narrow(0, 0, n_send).clone();
            }
        }
        Tensor uv_t = far.block(1, 2 * (int64_t)N).view({N, 2}).narrow(0, 0, V);
        Tensor mask_t = iar.block(6, (N + 3) / 4).view(torch::kBool).narrow(0, 0, N);
        ctx->saved_data["fr"] = guard;
        ctx->set_materialize_grads(false);
        ctx->mark_non_differentiable({mask_t});
        return {uv_t, mask_t};
    }

    static variable_list backward(AutogradContext* ctx, variable_list g) {
        variable_list out(7);
        FrameRec& fr = frame_of(ctx->saved_data["fr"].toTensor());
        if (!fr.owned_rows.defined() && !fr.gather_pending) {
            // the render node's backward did not run (no loss term on the image).  A loss on uv alone would be
            // dropped silently: its gradient reaches only the owned rows through the render node's exchange
            TORCH_CHECK(!g[0].defined(),
                        "sharded_rasterize: a gradient arrived on uv but none on the image; the owner-sliced frame "
                        "routes uv gradients through the image's backward -- put a (possibly zero-weight) loss term on the image");
            return out;
        }
        const auto dev = fr.xyz.device();
        const int n_sh = fr.n_sh;
        const ShardSpec& sp = fr.spec;
        Tensor owned = fr.owned_rows;
        fr.owned_rows = Tensor();
        Tensor recv = fr.recv_rows;
        fr.recv_rows = Tensor();
        bool gathered = fr.gather_pending;
        fr.gather_pending = false;
        // a loss term put directly on uv arrives on top of what node 2 handed over (the owned rows' uv columns,
        // or a stride-0 placeholder)
        const Tensor& g_uv = g[0];
        Tensor rendered = fr.rendered_uv_grad;
        fr.rendered_uv_grad = Tensor();
        const bool extra_uv = g_uv.defined() && fr.v_hi > fr.v_lo && g_uv.stride(0) != 0 &&
                              !(rendered.defined() && g_uv.unsafeGetTensorImpl() == rendered.unsafeGetTensorImpl());
        if (gathered && extra_uv) {
            // ... and needs the owned rows as a tensor after all
            const int64_t n_own = fr.v_hi - fr.v_lo;
            owned = torch::empty({std::max<int64_t>(n_own, 1), SLAB_WIDTH}, recv.options()).narrow(0, 0, n_own);
            void* stream = cur_stream();
            timed("gs_halo_gather_sum", stream, [&] {
                return gs_band_gather_sum(fr.halo_ws.data_ptr<int32_t>(), fr.N, sp.G, sp.rank, sp.owner_blocks.data(),
                                          fr.rank_t.data_ptr<int32_t>(), (int)fr.v_lo, recv.data_ptr(),
                                          fr.recv_offsets.data(), owned.data_ptr(), stream);
            });
            gathered = false;
        }
        if (extra_uv) {   // add the rest for the owned rows
            Tensor extra = g_uv.narrow(0, fr.v_lo, fr.v_hi - fr.v_lo);
            if (rendered.defined() && rendered.stride(0) != 0) extra = extra - rendered.narrow(0, fr.v_lo, fr.v_hi - fr.v_lo);
            owned = owned.clone();
            owned.narrow(1, 4, 2).add_(extra);
        }
        const int64_t n = fr.i1 - fr.i0;
        ParamGrads ga(dev, n, n_sh);
        if (n > 0) {
            void* stream = cur_stream();
            const int64_t i0 = fr.i0;
            timed("gs_preprocess_backward", stream, [&] {
                if (gathered)
                    return gs_preprocess_backward_gathered(
                        fr.xyz.data_ptr<float>() + 3 * i0, fr.quaternion.data_ptr<float>() + 4 * i0,
                        fr.scale.data_ptr<float>() + 3 * i0, n_sh, fr.camera_T_world.data_ptr(), fr.K.data_ptr(),
                        fr.center.data_ptr(), fr.rank_t.data_ptr<int32_t>() + i0, fr.opa_act.data_ptr(),
                        fr.halo_ws.data_ptr<int32_t>(), fr.N, sp.G, sp.rank, sp.owner_blocks.data(), recv.data_ptr(),
                        fr.recv_offsets.data(), (int)n, ga.ptr(0), ga.ptr(1), ga.ptr(2), ga.ptr(3), ga.ptr(4), ga.ptr(5),
                        stream);
                return gs_preprocess_backward_mode(
                    fr.xyz.data_ptr<float>() + 3 * i0, fr.quaternion.data_ptr<float>() + 4 * i0,
                    fr.scale.data_ptr<float>() + 3 * i0, n_sh, fr.camera_T_world.data_ptr(), fr.K.data_ptr(),
                    fr.center.data_ptr(), fr.rank_t.data_ptr<int32_t>() + i0, fr.opa_act.data_ptr(), owned.data_ptr(),
                    (int)fr.v_lo, (int)n, ga.ptr(0), ga.ptr(1), ga.ptr(2), ga.ptr(3), ga.ptr(4), ga.ptr(5), GS_RASTER_CLASSIC,
                    stream);
            });
        }
        ga.views(out);
        return out;
    }
};

struct OwnerRender : public torch::autograd::Function<OwnerRender> {
    static Tensor forward(AutogradContext* ctx, Tensor uv, Tensor guard) {
        FrameRec& fr = frame_of(guard);
        const ShardSpec& sp = fr.spec;
        ctx->saved_data["fr"] = guard;
        ctx->set_materialize_grads(false);
        Tensor image = fr.out.image;
        if (sp.a2a_hook.is_none() && sp.equal_bands) {
            // in-place all-gather of the equal bands: every rank's band sits at its own rows of the padded buffer
            const int64_t chunk = sp.band_pixel_rows * fr.W * 3;
            Tensor flat = image.view({-1}).narrow(0, 0, sp.G * chunk);
            Tensor mine = flat.narrow(0, sp.rank * chunk, chunk).clone();
            void* stream = cur_stream();
            timed_region("rccl_all_gather_image", stream, [&] { sp.pg->_allgather_base(flat, mine)->wait(); });
        } else if (sp.a2a_hook.is_none()) {
            // cost-balanced bands: chunks of chunk_rows pixel rows, the last one carrying this band's per-row costs;
            // the gathered chunks are assembled into the frame and the summed costs land in pinned host memory
            // (ShardedRasterizer reads them before the next frame: take_row_costs)
            void* stream = cur_stream();
            const int nty = (fr.H + 15) / 16, ntx = (fr.W + 15) / 16;
            const int64_t row_floats = 3 * (int64_t)fr.W, crows = sp.chunk_rows;
            float* base = image.data_ptr<float>();
            ok(gs_band_row_costs(fr.ranges.data_ptr<int32_t>(), ntx, nty, fr.row0, fr.row1, 64, GS_SORT_PREFIX,
                                 base + (16 * (int64_t)fr.row0 + crows - 1) * row_floats, stream));
            Tensor mine = image.view({-1}).narrow(0, 16 * (int64_t)fr.row0 * row_floats, crows * row_floats);
            Tensor gathered = torch::empty({sp.G * crows * row_floats}, image.options());
            timed_region("rccl_all_gather_image", stream, [&] { sp.pg->_allgather_base(gathered, mine)->wait(); });
            Tensor full = torch::empty({fr.H, fr.W, 3}, image.options());
            Tensor host_costs = torch::empty({nty}, torch::TensorOptions().dtype(torch::kFloat32).pinned_memory(true));
            ok(gs_band_assemble(gathered.data_ptr(), sp.bounds.data(), sp.G, (int)crows, fr.W, fr.H, nty, full.data_ptr(),
                                host_costs.data_ptr(), stream));
            hipEvent_t ev;
            hip_ok(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            hip_ok(hipEventRecord(ev, (hipStream_t)stream));
            {
                std::lock_guard<std::mutex> lock(g_mutex);
                RowCosts& rc = g_row_costs[(int)image.device().index()];
                if (rc.event) (void)hipEventDestroy(rc.event);
                rc.host = host_costs;
                rc.event = ev;
            }
            return full;
        }
        return image.narrow(0, 0, fr.H);
    }

    static variable_list backward(AutogradContext* ctx, variable_list g) {
        variable_list out(2);
        if (!g[0].defined()) return out;
        FrameRec& fr = frame_of(ctx->saved_data["fr"].toTensor());
        const ShardSpec& sp = fr.spec;
        const int W = fr.W, H = fr.H;
        const int64_t V = fr.V;
        Tensor grad_image = g[0].contiguous();
        Tensor slab = torch::empty({std::max<int64_t>(fr.L, 1), SLAB_WIDTH}, fr.packed.options());   // (zero_slab_rows)
        void* stream = cur_stream();
        const bool segmented = fr.out.seg.numel() > 0;
        timed("gs_render_backward_prologue", stream, [&] {
            return gs_render_backward_prologue(slab.data_ptr(), slab.size(0), nullptr, nullptr, W, H, fr.row0, fr.row1, stream);
        });
        timed("gs_render_tiles_backward_slab", stream, [&] {
            return gs_render_tiles_backward_slab_m(fr.packed.data_ptr(), fr.rgbr.data_ptr(), fr.ranges.data_ptr<int32_t>(),
                                                   fr.sorted_g.data_ptr<int32_t>(), fr.bg.data_ptr(), fr.out.nsp.data_ptr<int32_t>(),
                                                   fr.out.fw.data_ptr(), grad_image.data_ptr(), W, H, fr.row0, fr.row1,
                                                   slab.data_ptr(), 0, nullptr, nullptr,
                                                   segmented ? fr.out.seg.data_ptr() : nullptr, nullptr, nullptr, nullptr,
                                                   fr.bwd_mode,
                                                   fr.out.masks.defined() ? (const uint64_t*)fr.out.masks.data_ptr<int64_t>() : nullptr,
                                                   stream);
        });
        // rows of the send list -> owners; rows of the owned range <- the ranks whose band they reach
        int64_t n_send = 0, n_recv = 0;
        for (int64_t c : fr.send_splits) n_send += c;
        for (int64_t c : fr.recv_splits) n_recv += c;
        // (band-compact rows ARE the send list, in its order)
        Tensor send = fr.compact ? slab.narrow(0, 0, n_send) : slab.index_select(0, fr.halo_send.narrow(0, 0, n_send));
        Tensor recv = torch::empty({n_recv, SLAB_WIDTH}, slab.options());
        if (!sp.a2a_hook.is_none()) {
            py::gil_scoped_acquire gil;
            sp.a2a_hook(recv, send, fr.recv_splits, fr.send_splits);
        } else {
            timed_region("rccl_all_to_all_grad_rows", stream,
                         [&] { sp.pg->alltoall_base(recv, send, fr.recv_splits, fr.send_splits)->wait(); });
        }
        const int64_t n_own = fr.v_hi - fr.v_lo;
        std::vector<int32_t> offs(sp.G);
        {
            int32_t off = 0;
            for (int s2 = 0; s2 < sp.G; s2++) {
                offs[s2] = off;
                off += (int32_t)fr.recv_splits[s2];
            }
        }
        // uv.grad (trainer.py:360,379): the complete rows of the owned Gaussians, zeros elsewhere -- materialised
        // only when somebody retains it; a stride-0 zero routes the backward otherwise
        bool retained = false;
        if (auto impl = fr.uv_weak.lock()) retained = Tensor(std::move(impl)).retains_grad();
        Tensor owned;
        if (fr.fused && !retained) {
            // fused band frames: the per-Gaussian backward sums the received rows itself (no [owned, 9] round trip)
            fr.recv_rows = recv;
            fr.recv_offsets = offs;
            fr.gather_pending = true;
        } else {
            owned = torch::empty({std::max<int64_t>(n_own, 1), SLAB_WIDTH}, slab.options()).narrow(0, 0, n_own);
            if (n_own > 0) {
                timed("gs_halo_gather_sum", stream, [&] {
                    if (fr.fused)
                        return gs_band_gather_sum(fr.halo_ws.data_ptr<int32_t>(), fr.N, sp.G, sp.rank, sp.owner_blocks.data(),
                                                  fr.rank_t.data_ptr<int32_t>(), (int)fr.v_lo, recv.data_ptr(), offs.data(),
                                                  owned.data_ptr(), stream);
                    return gs_halo_gather_sum((const uint32_t*)fr.halo_mask.data_ptr<int32_t>(), fr.halo_ws.data_ptr<int32_t>(),
                                              fr.N, sp.G, sp.rank, (int)fr.v_lo, (int)fr.v_hi, recv.data_ptr(), offs.data(),
                                              owned.data_ptr(), stream);
                });
            }
            fr.owned_rows = owned;
        }
        Tensor g_uv;
        if (retained) {
            g_uv = torch::zeros({V, 2}, slab.options());
            if (n_own > 0) g_uv.narrow(0, fr.v_lo, n_own).copy_(owned.narrow(1, 4, 2));
        } else {
            g_uv = zero_scalar(slab.device()).expand({V, 2});
        }
        fr.rendered_uv_grad = g_uv;
        out[0] = g_uv;
        return out;
    }
};

std::tuple<Tensor, Tensor, Tensor> sharded_rasterize(
    Tensor o_xyz, Tensor o_quaternion, Tensor o_scale, Tensor o_opacity, Tensor o_rgb, c10::optional<Tensor> o_sh, Tensor xyz,
    Tensor quaternion, Tensor scale, Tensor opacity, Tensor rgb, c10::optional<Tensor> sh, Tensor camera_T_world, Tensor K,
    int64_t width, int64_t height, double near_thresh, double far_thresh, double cull_mask_padding, double mh_dist,
    Tensor background_rgb, int64_t world_size, int64_t rank, std::vector<int64_t> bounds, std::vector<int64_t> owner_blocks,
    py::object process_group, py::object all_to_all_hook, bool cost_bands) {
    const bool has_sh = check_frame_inputs(xyz, quaternion, scale, opacity, rgb, sh, camera_T_world, K, background_rgb, width, height);
    const auto dev = xyz.device();
    const int64_t N = xyz.size(0);
    const int G = (int)world_size, me = (int)rank;
    TORCH_CHECK(G >= 1 && G <= GS_MAX_RANKS && me >= 0 && me < G, "bad world size / rank");
    TORCH_CHECK((int)bounds.size() == G + 1 && (int)owner_blocks.size() == G + 1, "bounds / owner_blocks need world_size + 1 entries");
    const int64_t nty = (height + 15) / 16;
    auto fr = std::make_shared<FrameRec>();
    ShardSpec& sp = fr->spec;
    sp.G = G;
    sp.rank = me;
    for (int64_t b : bounds) sp.bounds.push_back((int32_t)b);
    for (int64_t b : owner_blocks) sp.owner_blocks.push_back((int32_t)b);
    sp.a2a_hook = all_to_all_hook;
    if (all_to_all_hook.is_none()) {
        TORCH_CHECK(!process_group.is_none(), "sharded_rasterize needs a process group (or the test hook)");
        sp.pg = process_group.cast<c10::intrusive_ptr<c10d::ProcessGroup>>();
        TORCH_CHECK(sp.pg->getSize() == G && sp.pg->getRank() == me, "process group does not match world_size / rank");
    }
    sp.band_pixel_rows = 16 * ((nty + G - 1) / G);
    sp.padded_height = sp.band_pixel_rows * G;
    {
        const int64_t rows_per = (nty + G - 1) / G;
        int64_t tallest = 0;
        for (int r = 0; r < G; r++) {
            TORCH_CHECK(sp.bounds[r] <= sp.bounds[r + 1], "bounds must be ascending");
            tallest = std::max<int64_t>(tallest, sp.bounds[r + 1] - sp.bounds[r]);
            sp.equal_bands = sp.equal_bands && sp.bounds[r] == std::min<int64_t>(nty, r * rows_per);
        }
        sp.equal_bands = sp.equal_bands && sp.bounds[G] == nty;
        TORCH_CHECK(sp.bounds[0] == 0 && sp.bounds[G] == nty, "bounds must cover the tile rows [0, ", nty, ")");
        // equal bands are gathered in place; the cost policy always gathers chunks (their last row is how the costs
        // travel), whatever this frame's split happens to be
        TORCH_CHECK(cost_bands || sp.equal_bands || !all_to_all_hook.is_none(),
                    "sharded_rasterize: unequal bands need cost_bands = true (the chunked image gather)");
        if (cost_bands) sp.equal_bands = false;
        sp.chunk_rows = 16 * tallest + 1;
        TORCH_CHECK(sp.equal_bands || nty <= 3 * width, "image too narrow for the cost row");
    }
    fr->row0 = sp.bounds[me];
    fr->row1 = sp.bounds[me + 1];
    TORCH_CHECK(0 <= fr->row0 && fr->row0 <= fr->row1 && fr->row1 <= nty, "bad tile row range");
    fr->xyz = xyz.contiguous();
    fr->quaternion = quaternion.contiguous();
    fr->scale = scale.contiguous();
    fr->opacity = opacity.contiguous();
    fr->rgb = rgb.contiguous();
    if (has_sh) fr->sh = sh->contiguous();
    fr->camera_T_world = camera_T_world.contiguous();
    fr->K = K.contiguous();
    fr->bg = background_rgb.contiguous();
    fr->N = (int)N;
    fr->n_sh = has_sh ? (int)sh->size(2) + 1 : 1;
    fr->W = (int)width;
    fr->H = (int)height;
    fr->near_thresh = near_thresh;
    fr->far_thresh = far_thresh;
    fr->padding = cull_mask_padding;
    fr->mh_dist = mh_dist;
    fr->i0 = (int)std::min<int64_t>(N, 256 * owner_blocks[me]);
    fr->i1 = (int)std::min<int64_t>(N, 256 * owner_blocks[me + 1]);
    TORCH_CHECK(o_xyz.size(0) == fr->i1 - fr->i0, "the owned slices do not match owner_blocks");
    c10::DeviceGuard dguard(dev);
    Tensor guard = make_guard(fr);
    auto o = OwnerPreprocess::apply(o_xyz, o_quaternion, o_scale, o_opacity, o_rgb, o_sh, guard);
    fr->uv_weak = c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl>(o[0].getIntrusivePtr());
    Tensor image = OwnerRender::apply(o[0], guard);
    return std::make_tuple(image, o[1], o[0]);
}

py::dict last_plan() {
    std::lock_guard<std::mutex> lock(g_mutex);
    py::dict d;
    d["v_lo"] = g_last_plan.v_lo;
    d["v_hi"] = g_last_plan.v_hi;
    d["V"] = g_last_plan.V;
    d["S"] = g_last_plan.S;
    d["send_splits"] = g_last_plan.send_splits;
    d["recv_splits"] = g_last_plan.recv_splits;
    d["L"] = g_last_plan.L;
    d["compact"] = g_last_plan.compact;
    if (g_keep_band_lists && g_last_plan.ranges.defined()) {
        d["ranges"] = g_last_plan.ranges;
        d["sorted_g"] = g_last_plan.sorted_g;
        d["send_list"] = g_last_plan.send_list;
    }
    return d;
}

py::dict counters() {
    std::vector<Tensor> log;
    Counters c;
    {
        std::lock_guard<std::mutex> lock(g_mutex);
        log = g_flag_log;
        c = g_counters;
    }
    int64_t repaired = 0;
    for (const Tensor& f : log) repaired += f.sum().item<int64_t>();
    py::dict d;
    d["frames"] = c.frames;
    d["speculative_frames"] = c.speculative;
    d["capacity_misses"] = c.misses;
    d["S_min"] = c.s_min < 0 ? py::object(py::none()) : py::object(py::int_(c.s_min));
    d["S_max"] = c.s_max < 0 ? py::object(py::none()) : py::object(py::int_(c.s_max));
    d["slab_copies"] = c.slab_copies;   // backward calls that could not read the render node's slab in place
    d["depth_cut_frames"] = c.cut_frames;
    d["depth_cut_backoffs"] = c.cut_backoffs;
    d["prefix_frames_without_repair_launches"] = c.render_only;   // no list beyond the prefix: render phase alone
    d["prefix_late_repairs"] = c.late_repairs;                    // guessed so, wrongly: repair enqueued after the host read
    d["long_list_misses"] = c.long_list_misses;                   // guessed "no list beyond 4096", wrongly: frame repeated
    d["prefix_repaired_tiles"] = repaired;
    d["prefix_frames_logged"] = (int64_t)log.size();
    return d;
}

void reset_counters() {
    std::lock_guard<std::mutex> lock(g_mutex);
    g_counters = Counters();
    g_flag_log.clear();
}

// every call drops what was kept
void keep_last_slab(bool on) {
    std::lock_guard<std::mutex> lock(g_mutex);
    g_keep_slab = on;
    g_last_slab = Tensor();
}
c10::optional<Tensor> last_slab() {
    std::lock_guard<std::mutex> lock(g_mutex);
    c10::optional<Tensor> out;
    if (g_last_slab.defined()) out = g_last_slab;
    return out;
}

c10::optional<Tensor> last_tile_flags(bool clear) {
    std::lock_guard<std::mutex> lock(g_mutex);
    c10::optional<Tensor> out;
    if (g_last_flags.defined()) out = g_last_flags;
    if (clear) g_last_flags = Tensor();
    return out;
}

void enable_timing(bool on, const std::string& only) {
    std::lock_guard<std::mutex> lock(g_mutex);
    g_timing.on = on;
    g_timing.only = only;
}

void reserve_events(int64_t n) {
    std::lock_guard<std::mutex> lock(g_mutex);
    while ((int64_t)g_timing.pool.size() < n) {
        hipEvent_t e;
        hip_ok(hipEventCreate(&e));
        g_timing.pool.push_back(e);
    }
}

py::dict collect_timing() {
    hip_ok(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lock(g_mutex);
    py::dict d;
    for (auto& kv : g_timing.spans) {
        py::list ms;
        for (auto& ab : kv.second) {
            float t = 0;
            hip_ok(hipEventElapsedTime(&t, ab.first, ab.second));
            ms.append(t);
            g_timing.pool.push_back(ab.first);
            g_timing.pool.push_back(ab.second);
        }
        d[py::str(kv.first)] = ms;
    }
    g_timing.spans.clear();
    return d;
}

// cost-balanced bands: the per-row costs the latest frame's image gather left behind (None if there are none); waits
// for the kernel that wrote them, which has long finished when the next frame asks
py::object take_row_costs() {
    Tensor host;
    hipEvent_t ev = nullptr;
    {
        // the costs of the CURRENT device's latest frame (one slot per device)
        int dev = 0;
        hip_ok(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lock(g_mutex);
        RowCosts& rc = g_row_costs[dev];
        host = rc.host;
        ev = rc.event;
        rc.host = Tensor();
        rc.event = nullptr;
    }
    if (!host.defined()) return py::none();
    if (ev) {
        hip_ok(hipEventSynchronize(ev));
        (void)hipEventDestroy(ev);
    }
    py::list out;
    const float* p = host.data_ptr<float>();
    for (int64_t i = 0; i < host.numel(); i++) out.append(p[i]);
    return out;
}

// tests: shrink / grow every stored capacity guess (a too small one must be detected and the frame's emit, sort and
// render repeated with the exact sizes)
void debug_scale_capacity_hints(double factor) {
    std::lock_guard<std::mutex> lock(g_mutex);
    for (auto& kv : g_shapes)
        for (auto* c : {&kv.second.capacity[0], &kv.second.capacity[1], &kv.second.overflow_capacity})
            if (*c) *c = (int64_t)(**c * factor);
}

// (tests) overwrite the longest-list guesses of every shape seen so far
void debug_set_longest_list_hints(int64_t value) {
    std::lock_guard<std::mutex> lock(g_mutex);
    for (auto& kv : g_shapes)
        if (kv.second.longest_list) kv.second.longest_list = value;
}

void set_segments(int mode) { g_policy.segments = mode; }
void set_depth_cut(int mode, int64_t min_mean_list) {
    g_policy.depth_cut = mode;
    if (min_mean_list > 0) g_policy.cut_min_mean_list = min_mean_list;
}
void set_band_compact(bool on) { g_band_compact = on; }
void set_band_fused(bool on) { g_band_fused = on; }
void set_touch_masks(bool on) { g_touch_masks = on; }

void set_modes(bool sort_prefix, bool early_render) {
    g_policy.sort_prefix = sort_prefix;
    g_policy.early_render = early_render;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "native orchestration of the fused MI355X rasterization frame (see gaussian_splatting_amd/fused.py)";
    m.def("rasterize", &rasterize, "fused frame: -> (image, culling_mask, uv)", py::arg("xyz"), py::arg("quaternion"),
          py::arg("scale"), py::arg("opacity"), py::arg("rgb"), py::arg("sh"), py::arg("camera_T_world"), py::arg("K"),
          py::arg("width"), py::arg("height"), py::arg("near_thresh"), py::arg("far_thresh"), py::arg("cull_mask_padding"),
          py::arg("mh_dist"), py::arg("background_rgb"), py::arg("row0") = 0, py::arg("row1") = -1,
          py::arg("raster_mode") = (int64_t)GS_RASTER_CLASSIC, py::arg("filter3d") = py::none());
    m.def("rasterize_adam", &rasterize_adam,
          "fused frame whose backward steps quaternion, scale, opacity, rgb and sh (Adam) itself: -> (image, culling_mask, uv)",
          py::arg("xyz"), py::arg("quaternion"), py::arg("scale"), py::arg("opacity"), py::arg("rgb"), py::arg("sh"),
          py::arg("camera_T_world"), py::arg("K"), py::arg("width"), py::arg("height"), py::arg("near_thresh"),
          py::arg("far_thresh"), py::arg("cull_mask_padding"), py::arg("mh_dist"), py::arg("background_rgb"), py::arg("plan"));
    m.def("sharded_rasterize", &sharded_rasterize,
          "one rank of the tile-row sharded frame, owner-sliced gradients, equal or cost-balanced bands: -> (image, culling_mask, uv)");
    m.def("last_plan", &last_plan);
    m.def("debug_keep_band_lists", [](bool on) {
        std::lock_guard<std::mutex> lock(g_mutex);
        g_keep_band_lists = on;
        if (!on) g_last_plan.ranges = g_last_plan.sorted_g = g_last_plan.send_list = Tensor();
    }, py::arg("on"));
    m.def("take_row_costs", &take_row_costs);
    m.def("counters", &counters);
    m.def("reset_counters", &reset_counters);
    m.def("set_modes", &set_modes, py::arg("sort_prefix"), py::arg("early_render"));
    m.def("set_segments", &set_segments, py::arg("mode"));
    m.def("debug_scale_capacity_hints", &debug_scale_capacity_hints, py::arg("factor"));
    m.def("debug_set_longest_list_hints", &debug_set_longest_list_hints, py::arg("value"));
    m.def("set_depth_cut", &set_depth_cut, py::arg("mode"), py::arg("min_mean_list") = 0);
    m.def("set_band_compact", &set_band_compact, py::arg("on"));
    m.def("set_band_fused", &set_band_fused, py::arg("on"));
    m.def("set_touch_masks", &set_touch_masks, py::arg("on"));
    if (const char* e = std::getenv("GSPLAT_TOUCH_MASKS")) g_touch_masks = std::atoi(e) != 0;   // (A/B runs of bench.py)
    m.def("last_tile_flags", &last_tile_flags, py::arg("clear") = false);
    m.def("keep_last_slab", &keep_last_slab, py::arg("on"));
    m.def("last_slab", &last_slab);
    m.def("note_slab", &note_slab, py::arg("slab"));
    m.def("enable_timing", &enable_timing, py::arg("on"), py::arg("only") = std::string());
    m.def("reserve_events", &reserve_events);
    m.def("collect_timing", &collect_timing);
}
