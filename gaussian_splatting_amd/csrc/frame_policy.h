// frame_policy.h -- what the native frame (frame_hip.cpp) remembers about a frame shape and the host-side decisions it
// takes from that, as pure functions of a handful of integers (standard library only: no torch, no HIP).  A frame reads
// its shape's record at its start (want_depth_cut, plan_frame), the frame's counts from the device once, and writes the
// record after that (classify_frame, learn, segments_for).
#ifndef GSPLAT_FRAME_POLICY_H
#define GSPLAT_FRAME_POLICY_H
#include <algorithm>
#include <cstdint>
#include <optional>

namespace frame_policy {
constexpr int PREFIX_RENDER = 1, PREFIX_REPAIR = 2;   // = GS_PREFIX_RENDER, GS_PREFIX_REPAIR (include/gsplat_hip.h)
constexpr int CUT_COOLDOWN = 32;

// the process-wide switches (gsplat_frame.set_modes / set_segments / set_depth_cut)
struct Policy {
    bool sort_prefix = true, early_render = true;
    // depth segments of the backward (include/gsplat_hip.h: gs_render_segment_workspace_bytes): 0 = auto (frames /
    // bands of fewer than 1500 tiles whose lists average >= 192 entries: a multi-GPU rank's band), 1 = always, -1 = never
    int segments = 0;
    // depth cut: 0 = auto (whole frames in the LDS-histogram regime whose lists averaged cut_min_mean_list entries or
    // more in an earlier frame of the same shape), 1 = always (where supported), -1 = never
    int depth_cut = 0;
    int64_t cut_min_mean_list = 1280;   // workload C (1477 per tile): 1.227 -> 1.193 ms with the cut (profiles/r04)
};

// One record per frame shape (device, N, tiles, tile rows): every guess a frame of that shape takes from earlier ones.
// An empty optional is "not yet known", which is not a guess of 0: a frame without a capacity guess is not speculative.
// Single-GPU frames and band frames of the same shape share the record.
struct ShapeState {
    // instance capacity of the lists, [0] complete lists, [1] depth-cut lists (their kept count is another quantity)
    std::optional<int64_t> capacity[2];
    // longest tile list of the shape's last complete-list frame (a guess for the next; cut frames do not report one)
    std::optional<int64_t> longest_list;
    // depth cut (include/gsplat_hip.h "depth-bucketed binning"): capacity of the overflow buffers (the frame's complete
    // instance count) and the complete instance count of the latest frame of the shape (what "auto" decides on)
    std::optional<int64_t> overflow_capacity, complete_count;
    std::optional<int64_t> visible_count;   // V of the shape's latest frame (the cut's partition scales with V, not N)
    // "auto" segments are decided ONCE per frame shape, from the exact instance count of the first frame of that shape
    // (which is never speculative), and kept: a speculative frame only knows a capacity (S * 1.25 + 4096), so near the
    // 192-entries-per-tile threshold the first frame and later frames of the same scene would pick different backward
    // kernels and their gradients would differ in the last bits from frame to frame (round-3 advisor finding).
    std::optional<bool> segment_choice;
    // "auto" cut also backs off when the cut does not pay: a frame in which more than an eighth of the tiles had to be
    // repaired from their complete lists (faint scenes, e.g. right after an opacity reset: every pixel composites deep)
    // emitted most lists twice.  The render's repair kernel leaves the flagged-tile count of every cut frame in a pinned
    // word (kept next to this record); it is looked at -- never waited for -- when a later frame of the shape decides,
    // and switches the cut off for the next CUT_COOLDOWN frames of that shape (then it is tried again).
    int cut_cooldown = 0;
};

inline bool want_segments(const Policy& p, int64_t n_instances, int64_t n_tiles) {
    if (p.segments == 0) return n_tiles > 0 && n_tiles < 1500 && n_instances >= 192 * n_tiles;
    return p.segments > 0 && n_tiles > 0;
}

// the backward of a complete-list frame; exact_count: n_instances is the frame's count, not a capacity (may be stored)
inline bool segments_for(ShapeState& st, const Policy& p, int64_t n_instances, bool exact_count, int64_t n_tiles) {
    if (p.segments != 0) return want_segments(p, n_instances, n_tiles);
    if (st.segment_choice) return *st.segment_choice;
    const bool on = want_segments(p, n_instances, n_tiles);
    if (exact_count) st.segment_choice = on;
    return on;
}

struct CutDecision {
    bool cut = false;
    // the backoff ended: the caller zeroes the pinned feedback word | a backoff started (counter depth_cut_backoffs)
    bool clear_word = false, backoff = false;
};
// Does this frame take the depth cut?  supported(n) = gs_cut_supported(ntx, row0, row1, n); flagged_word = the shape's
// pinned feedback word as it reads now (0 while the shape has none).
template <typename Supported>
CutDecision want_depth_cut(ShapeState& st, const Policy& p, int N, int64_t n_tiles, bool whole, int sort_prefix,
                           int32_t flagged_word, Supported&& supported) {
    CutDecision d;
    if (p.depth_cut < 0 || !whole || !sort_prefix) return d;
    if (!supported(N)) return d;
    if (p.depth_cut > 0) {
        d.cut = true;
        return d;
    }
    if (!st.complete_count || *st.complete_count < p.cut_min_mean_list * n_tiles) return d;
    // gs_cut_supported gates on N, the capacity; what the cut's partition and count passes walk is the VISIBLE set: a
    // heavily culled view of a large scene can pass the gate on N and not pay (round-4 advisor finding)
    if (st.visible_count && !supported((int)std::min<int64_t>(*st.visible_count, N))) return d;
    // "auto" cut and "auto" segments exclude each other per shape: a cut frame takes the unsegmented backward, so a
    // small whole frame that qualifies for both (fewer than 1500 tiles, long lists) would otherwise change backward
    // kernels -- and the last bits of its gradients -- whenever the cut policy switches (first frame of a shape,
    // every backoff).  Such shapes keep the segments (round-4 advisor finding).
    // What counts is what the backward of this shape will really take: the choice segments_for() STORED from the
    // shape's first exact count when there is one (a shape whose lists grew past the cut's threshold later -- a
    // densifying scene -- keeps its stored "no segments" and may take the cut), want_segments() on the latest
    // complete count only before that.  Segments FORCED on (p.segments > 0) are an explicit request for the
    // segmented backward, which a cut frame cannot honour: the auto cut then stays off (round-5 advisor finding).
    if (p.segments > 0) return d;
    if (p.segments == 0 && (st.segment_choice ? *st.segment_choice : want_segments(p, *st.complete_count, n_tiles))) return d;
    // During a backoff no cut frame is enqueued, so the word is not looked at; it is cleared when the backoff
    // ends -- CUT_COOLDOWN uncut frames after the last cut frame was enqueued, whose repair kernel has long
    // written its count by then -- never while a cut frame may still be in flight (a count landing after a
    // host-side reset used to start a second backoff; round-4 advisor finding).
    if (st.cut_cooldown > 0) {
        d.clear_word = --st.cut_cooldown == 0;
        return d;
    }
    if ((int64_t)flagged_word * 8 > n_tiles) {
        st.cut_cooldown = CUT_COOLDOWN;
        d.backoff = true;
        return d;
    }
    d.cut = true;
    return d;
}

// ---- one frame: the plan before the host read, the classification after it ------------------------------------
struct FrameKind {
    bool cut;             // depth-cut lists
    int sort_prefix;      // GS_SORT_PREFIX, or 0: lists sorted in full
    bool guess_longest;   // the count pass reports the longest list and the frame guesses it (complete lists in prefix mode)
    bool split_repair;    // the render may go without its repair phase and get it late (single-GPU frames; not bands)
};
struct FramePlan {
    // with capacities guessed from earlier frames of the shape, emit + sort + render are enqueued before the host waits
    bool speculative = false;
    int64_t capacity = 0, overflow_capacity = 0;
    // Complete-list frames also guess the LONGEST list (from the shape's last frame): none beyond 4096 entries ->
    // the sort's walk-grid kernel for those is not enqueued, none beyond the prefix -> neither is the render's
    // repair phase (a sparse frame -- workload B -- otherwise pays ~5 us each for three kernels that find nothing
    // to do).  The count pass's scan reports the true value with the frame's counts; a guess that was too small
    // is made good after the host read: the repair enqueued late, or emit + sort + render repeated.
    int64_t longest_guess = -1;
    bool early_render = false;
    int phases = PREFIX_RENDER | PREFIX_REPAIR;   // of the early render
};
inline FramePlan plan_frame(const ShapeState& st, const Policy& p, const FrameKind& k) {
    FramePlan f;
    f.speculative = st.capacity[k.cut] && (!k.cut || st.overflow_capacity);
    if (!f.speculative) return f;
    f.capacity = *st.capacity[k.cut];
    f.overflow_capacity = st.overflow_capacity.value_or(0);
    if (k.guess_longest && st.longest_list) f.longest_guess = *st.longest_list;
    f.early_render = p.early_render && k.sort_prefix && (k.cut || f.capacity > k.sort_prefix);
    if (f.early_render && k.split_repair && f.longest_guess >= 0 && f.longest_guess <= k.sort_prefix) f.phases = PREFIX_RENDER;
    return f;
}

// the frame's host read: S (depth cut: the kept count), the complete instance count, the longest list (-1: not reported)
struct FrameCounts {
    int64_t S, S_complete, longest;
};
enum class Act { Nothing, Render, LateRepair };
struct FrameOutcome {
    // a list beyond 4096 entries whose sort kernel was not enqueued: the lists are not what the render needs
    bool unsorted_long = false;
    bool miss = false;      // a guess was too small
    bool re_emit = false;   // emit + sort (again) with the exact sizes; the early render, if any, is void
    // Render: with the exact lists, now; LateRepair: the early render went without its repair phase and a list IS
    // longer than the prefix
    Act act = Act::Nothing;
    int phases = PREFIX_RENDER | PREFIX_REPAIR;   // what the frame's image went through in the end
    bool render_only = false;                     // counter: a prefix frame without repair launches
};
inline FrameOutcome classify_frame(const FramePlan& f, const FrameKind& k, const FrameCounts& c) {
    FrameOutcome o;
    o.unsorted_long = f.speculative && f.longest_guess >= 0 && f.longest_guess <= 4096 && c.longest > 4096;
    o.miss = f.speculative && (c.S > f.capacity || (k.cut && c.S_complete > f.overflow_capacity) || o.unsorted_long);
    o.re_emit = !f.speculative || o.miss;
    bool prefix_render;   // the image comes from the prefix render kernel (which has the two phases)
    if (!f.early_render || o.re_emit) {
        o.act = Act::Render;
        if (k.split_repair && !k.cut && k.sort_prefix && c.longest >= 0 && c.longest <= k.sort_prefix) o.phases = PREFIX_RENDER;
        prefix_render = !k.cut && k.sort_prefix && c.S > k.sort_prefix;
    } else {
        o.phases = f.phases;
        prefix_render = !k.cut;   // (an early render of complete lists: capacity > sort_prefix)
        if (!k.cut && f.phases == PREFIX_RENDER && c.longest > k.sort_prefix) {
            o.act = Act::LateRepair;
            o.phases = PREFIX_RENDER | PREFIX_REPAIR;
        }
    }
    o.render_only = o.phases == PREFIX_RENDER && prefix_render;
    return o;
}

// a capacity guess is the running maximum of the counts seen, with a quarter + 4096 entries of headroom
inline int64_t grown_capacity(int64_t old, int64_t S) { return std::max(old, S + S / 4 + 4096); }
// what a frame leaves in its shape's record for the next one
inline void learn(ShapeState& st, const FrameKind& k, const FrameCounts& c) {
    st.capacity[k.cut] = grown_capacity(st.capacity[k.cut].value_or(0), c.S);
    if (k.cut) st.overflow_capacity = grown_capacity(st.overflow_capacity.value_or(0), c.S_complete);
    if (k.guess_longest) st.longest_list = c.longest;
}

}  // namespace frame_policy
#endif
