// The body of the fused fp32 colour backward: ONE text of the walk, included by k_render_bwd<float, 1> (GS_BWD_ABS 0)
// and by k_render_bwd_abs (GS_BWD_ABS 1) in render.hip, which describes both.  Not a function: inlined from a shared
// __device__ routine the plain kernel came out with the same 1275 instructions in another register assignment and
// schedule, and its machine code is not to move (scripts/kernel_isa_diff.py); with GS_BWD_ABS 0 the preprocessor leaves
// the tokens the kernel has always had.  Expects the kernel's parameters by name (packed ... touch_masks, and g_uv_abs
// with GS_BWD_ABS 1).
    constexpr int REF_CH = ref_chunk<float>(1);
    // Every wave owns a slot of nine sums per staged splat and writes it once (plain store after a full-wave
    // reduction), the flush adds the slots of the waves that wrote -- no LDS atomics, no zero fill.
    constexpr int SV = 9;   // width of a slot: colour 3 | w, w du, w dv | conic terms 3
    constexpr int RCHUNK = GS_BWD_CHUNK;
    constexpr int NWORD = RCHUNK / 64 > 0 ? RCHUNK / 64 : 1;
    __shared__ alignas(16) float s_geom[RCHUNK * GS_PACKED_WIDTH];
    __shared__ int s_idx[RCHUNK];
    __shared__ float s_acc[4 * RCHUNK * SV];                     // [wave][splat][9]
    __shared__ int s_max[4];
    __shared__ unsigned long long s_mask[4][NWORD];
    __shared__ unsigned long long s_hit[4][NWORD];               // slots written by each wave
#if GS_BWD_ABS
    __shared__ float s_abs[4 * RCHUNK * 2];                      // [wave][splat][2]: the absgrad pair
#endif

    // depth segments (fused renderer, seg.rec != nullptr): work item = (tile, segment), block index =
    // segment * grid + block of the tile; segment 0 -- every pixel active, the most work -- starts first
    int seg_id = 0, blk = blockIdx.x;
    const bool seg_on = seg.rec != nullptr;
    if (seg_on) {
        const int g0 = render_grid(nt);
        seg_id = blockIdx.x / g0;
        blk = blockIdx.x - seg_id * g0;
    }
    const int t_local = tile_order ? tile_order[blk] : tile_of_block(blk, nt);
    if (t_local < 0 || t_local >= nt) return;
    const int tile = tile0 + t_local;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PixelMap px = pixel_of_thread(tile % ntx, tile / ntx, tid);
    const bool valid = px.u < W && px.v < H;
    int s0 = ranges[tile];
    int n_tile = ranges[tile + 1] - s0;
    // depth cut: a tile the forward had to redo from its complete list reads that list from the overflow buffer
    if (cut_flags != nullptr && cut_flags[tile] != 0) {
        s0 = full_ranges[tile];
        n_tile = full_ranges[tile + 1] - s0;
        sorted = overflow_sorted;
    }
    if (n_tile <= 0) return;

    int nsp = 0;
    float weight = 0;
    float gi[3] = {0, 0, 0};
    int kend = 0;                 // segments: index after the pixel's last contributor, and what the backward's
    float oma_last = 1, bgw = 0;  // first step at that splat does (written by the forward's epilogue)
    if (valid) {
        const size_t p = (size_t)px.v * W + px.u;
        nsp = nsp_in[p];
        weight = fw_in[p];
        if (seg_on) {
            kend = seg.kend[p - seg.pix0];
            oma_last = seg.oma_last[p - seg.pix0];
            bgw = seg.bgw[p - seg.pix0];
        }
        gi[0] = grad_image[p * 3 + 0];
        gi[1] = grad_image[p * 3 + 1];
        gi[2] = grad_image[p * 3 + 2];
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
#if GS_BWD_ABS
    const bool pair_stores = (lane & ~16) == 0;   // lanes 0 and 16 (reduce2_to_slot)
    const int pair_lane_base = wave * RCHUNK * 2 + ((lane >> 4) & 1);
#endif
    float color_accum[3] = {0, 0, 0};
    bool bg_init = false;
    const float bg0 = bg[0], bg1 = bg[1], bg2 = bg[2];

    GS_STAT_DECL;
    GS_HALF_DECL;
    GS_STAT(0, 1);          // waves
    GS_STAT(7, n_tile);
    GS_STAT(8, n_used);
    // the workgroup's part of the list: [seg_lo, seg_hi) (the whole used part without segments)
    int seg_lo = 0, seg_hi = n_used;
    int reach_end = nsp;   // the lane looks at list entries k < reach_end (render_backward.cu:131)
    if (seg_on) {
        seg_lo = seg_id * SEG_LEN;
        if (seg_lo >= n_used) return;
        if (seg_id < SEG_MAX - 1) seg_hi = min(n_used, seg_lo + SEG_LEN);
        if (kend <= seg_lo) {
            reach_end = 0;   // the pixel's walk ended in front of this segment
        } else if (kend > seg_hi) {
            // the pixel's walk comes from behind: resume it with the state it has at the boundary
            const Vec4<float>* rec = seg.rec + (size_t)(tile - seg.tile0) * SEG_MAX * RB + tid;
            const int e_p = min((kend - 1) / SEG_LEN, SEG_MAX - 1);        // segment of its last contributor
            const int e_tile = min((n_used - 1) / SEG_LEN, SEG_MAX - 1);   // wave-uniform bound
            const int k_m = kend - 1;
            const bool first_divides = (exact ? k_m : k_m % REF_CH) < nsp - 1;   // Q1 at the first contributor
            // weight after the walk's first step, with the last contributor's own factor taken out again
            // (it is inside P of its segment)
            float wb = (first_divides ? weight * fast_rcp(oma_last) : weight) * oma_last;
            float d0 = 0, d1 = 0, d2 = 0;
            for (int s2 = e_tile; s2 > seg_id; s2--) {   // deepest first, as the walk accumulates
                if (s2 <= e_p) {
                    const Vec4<float> r4 = rec[s2 * RB];
                    wb = wb * fast_rcp(r4.x);   // the walk's weight at the near boundary of segment s2
                    d0 += wb * r4.y; d1 += wb * r4.z; d2 += wb * r4.w;
                }
            }
            weight = wb;
            color_accum[0] = bg0 * bgw + d0;
            color_accum[1] = bg1 * bgw + d1;
            color_accum[2] = bg2 * bgw + d2;
            bg_init = true;
        }
    }
    const int first_chunk = seg_lo / RCHUNK;
    const int last_chunk = (seg_hi - 1) / RCHUNK;
    // Q1 (render_backward.cu:185 compares a chunk-local index): k % REF_CH for k = base + i, i < RCHUNK <= REF_CH, is
    // base % REF_CH + i with at most one wrap -- one scalar division per CHUNK instead of a multiply-high sequence
    // (9 scalar instructions) per visit; exact mode never wraps
    static_assert(RCHUNK <= REF_CH, "one wrap per chunk");
    const int q1_wrap = exact ? 0x7fffffff : REF_CH;
    const int prio_from = seg_on ? 0x7fffffff : first_chunk + 2;   // (wave priority, below)
    for (int chunk = last_chunk; chunk >= first_chunk; chunk--) {
        const int base = chunk * RCHUNK;
        const int base_q = exact ? base : base % REF_CH;
        const int cnt = min(RCHUNK, seg_hi - base);
        // Position in the walk sets the wave priority: 1 while more than two chunks of the list lie ahead, 0 for the last
        // two.  Deep in the list few lanes contribute and a visit is a dependent chain that wants its issue slot at once;
        // the last chunks (the front of the list, most lanes contributing) are dense vector work that fills the slots
        // left over.  A SIMD arbitrates vector issue by priority, then age: without this the old waves -- the ones in
        // their dense front chunks -- win (profiles/r15/render_wave_priority_ab.txt).  Loop counters only: one scalar
        // compare per chunk around the s_setprio, nothing per visit.  (Depth segments, two chunks each, stay at 0.)
        if (chunk >= prio_from) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
        GS_STAT(1, 1);
        __syncthreads();   // previous chunk fully flushed
        stage_chunk<float, 1, 1>(packed, rgb, sorted, s0 + base, cnt, tid, s_geom, nullptr, s_idx, src_opacity, src_conic);
        GS_PHASE(0);
        if constexpr (RCHUNK == 64) {
            if (touch_masks != nullptr && chunk < GS_MASK_WORDS) {
                // the forward's own masks of this word (GS_MASK_WORDS); entries beyond the used part are not staged here
                if (tid < 4) {
                    const unsigned long long keep = cnt >= 64 ? ~0ull : ((1ull << cnt) - 1);
                    s_mask[tid][0] = touch_masks[((size_t)tile * GS_MASK_WORDS + chunk) * 4 + tid] & keep;
                }
            } else {
                // one patch per wave (round 6): the records wave 0 staged have to be visible to the other three first
                __syncthreads();
                build_touch_masks_by_patch(s_geom, cnt, tid, tile % ntx, tile / ntx, s_mask);
            }
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
            const bool reach = k < reach_end;   // render_backward.cu:131 (nsp == 0 outside the image)
            GS_STAT(2, 1);                          // visits
            if (ballot(reach) == 0) continue;      // wave-uniform: no lane reaches this splat
            GS_STAT(9, 1);                          // visits with a reaching lane
            GS_STAT(6, __popcll(ballot(reach)));
            GS_STAT_FLAG(st_in);
            // ---- the visit ----
            // Per lane: aw = alpha * weight (colour gradient = aw * Y0 grad_image[ch]),
            // w = norm_prob * grad_alpha (the opacity gradient term), and with t = k w,
            // k = -0.5 opacity / det a per-splat constant applied in the flush:
            //   grad_u = -2 (c du - b dv) t, grad_v = -2 (a dv - b du) t     (render_backward.cu:216-219)
            //   grad_conic = (dv^2 - c mh, b mh - du dv, du^2 - a mh) t      (:221-229, cf = mh / det)
            // The uv pair only needs the sums of w du and w dv (the flush forms the combinations);
            // the conic terms are formed per pixel as the reference does -- their cancellation is
            // benign there and would not be after the sum.  All nine are 0 for a lane that does not
            // contribute, so the reduction needs no zero-filled value array.
            const float* rec = s_geom + i * GS_PACKED_WIDTH;
            const Vec4<float> g0 = *reinterpret_cast<const Vec4<float>*>(rec);       // u v r2 opacity
            // the whole 48-byte record at once (one LDS round trip per visit instead of three dependent
            // ones; LDS bandwidth is no longer what bounds this kernel): 0.70 -> 0.69 ms
            const Vec4<float> g1 = *reinterpret_cast<const Vec4<float>*>(rec + 4);   // a b c det
            const Vec4<float> g2 = *reinterpret_cast<const Vec4<float>*>(rec + 8);   // 1/det, colour
            asm volatile("" ::"v"(g1.x), "v"(g1.y), "v"(g1.z), "v"(g1.w), "v"(g2.x), "v"(g2.y), "v"(g2.z), "v"(g2.w));
            const float du = pu - g0.x, dv = pv - g0.y;
            const float du2 = du * du, dv2 = dv * dv;
            // aw, w and mh are formed by the lanes that pass the alpha test only; the others are cut out of the
            // nine sums by `contrib` below -- no zero-filled registers in front of (and, for the ones the
            // exponential reuses, again inside) the branches: they were 11 of the visit's ~120 vector instructions
            float aw = unset(), w = unset(), mh = unset(), duv = unset();
            bool contrib = false;
            if (reach && !(du2 + dv2 > g0.z)) {   // inside the cutoff radius
                GS_STAT_SET(st_in);
                // render_backward.cu:153-165 (multiplies by 1/det; the forward divides)
                duv = du * dv;
                mh = (g1.z * du * du - g1.w * du * dv + g1.x * dv * dv) * g2.x;   // g1.w = b + b (stage_chunk)
                // norm_prob = 0 unless mh > 0 (render_backward.cu:158-165) -- and then alpha = 0 fails the 1/255 test:
                // `mh > 0` joins the test's lane mask (a scalar and), behind it norm_prob IS the exponential
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
                        // grad_alpha (render_backward.cu:196-203); the record's colour is Y0 * coefficient
                        const float ga = (g2.y * weight - color_accum[0] * r1ma) * gi[0] +
                                         (g2.z * weight - color_accum[1] * r1ma) * gi[1] +
                                         (g2.w * weight - color_accum[2] * r1ma) * gi[2];
                        color_accum[0] += g2.y * aw;
                        color_accum[1] += g2.z * aw;
                        color_accum[2] += g2.w * aw;
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
            const float awy = awz * float(GS_SH_0);   // Y0 (the compiler re-formed Y0 * gi[ch] at every visit to save registers)
            val[0] = awy * gi[0]; val[1] = awy * gi[1]; val[2] = awy * gi[2];
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
#if GS_BWD_ABS
            {
                // the magnitudes of this visit's terms of grad_u, grad_v (wz = 0 where the lane does not contribute;
                // g1.y = b); -ffp-contract=off: two products, a difference, a product, the sign bit dropped
                const float e_u = fabsf(wz * (g1.z * du - g1.y * dv));
                const float e_v = fabsf(wz * (g1.x * dv - g1.y * du));
                reduce2_to_slot(e_u, e_v, pair_stores, s_abs, pair_lane_base + i * 2);
            }
#endif
            hit |= 1ull << bit;
          }
          if (lane == 0) s_hit[wave][word] = hit;
        }
        GS_PHASE(2);
        GS_HALF_CHUNK(12);
        __syncthreads();
        GS_PHASE(3);
        // the flush: one global atomic per value per (splat, tile)
        // Phase 1, thread = splat: flush_sum_slots' text, written out -- called as the routine, the same instructions
        // come out with a lane-mask merge of the visit loop scheduled four places later, and this kernel's visit loop
        // is not to move for a tidier flush.  A change to either is a change to both.
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
            // sums of (w, w du, w dv) and of the per-pixel conic terms -> gradients (see the loop).  A splat no wave
            // hit keeps its zeros unscaled: a record whose fp32 determinant cancelled to 0 carries 1 / det = inf (and
            // r2 = inf: it is staged in every tile), nobody can hit it (mh = q * inf never passes the alpha test), and
            // 0 * inf would flush NaN where the reference leaves its zeros.  A splat that was hit has a finite 1 / det.
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
#if GS_BWD_ABS
            {
                // the pair: the same waves' slots in the same order, times opacity |1 / det|
                float eu = 0, ev = 0;
#pragma unroll
                for (int w4 = 0; w4 < 4; w4++) {
                    if ((s_hit[w4][tid >> 6] >> (tid & 63)) & 1ull) {
                        eu += s_abs[(w4 * RCHUNK + tid) * 2 + 0];
                        ev += s_abs[(w4 * RCHUNK + tid) * 2 + 1];
                    }
                }
                // (as k above: zeros stay zeros; |1 / det|: a record whose fp32 determinant came out negative is
                // taken where form / det > 0, and these are sums of magnitudes)
                const float od = any_hit ? rec[3] * fabsf(rec[8]) : 0.0f;
                s_abs[tid * 2 + 0] = eu * od;
                s_abs[tid * 2 + 1] = ev * od;
            }
#endif
        }
        __syncthreads();
#if GS_BWD_ABS
        {
            // the pair's Phase 2, thread = value: consecutive addresses within a row, rows of two zeros untouched
            for (int j = tid; j < cnt * 2; j += RB) {
                const float v = s_abs[j];
                if (v != 0.0f || s_abs[j ^ 1] != 0.0f) global_add(g_uv_abs + (size_t)s_idx[j >> 1] * 2 + (j & 1), v);
            }
        }
#endif
        // Phase 2, nine lanes = one row: a wave's atomic instruction then covers seven whole 36-byte
        // rows with consecutive addresses, which the L2 handles per cache line -- 6x the rate of one
        // thread per row with nine instructions (scripts/ubench/atomic_rows.hip: 0.094 vs 0.557 ms for
        // the 1.25 M rows of a frame; the per-row form had become 0.17 ms of this kernel).
        const int sub = lane / SV, col = lane - sub * SV;   // lane 63: idle
        for (int r0 = wave * 7; r0 < cnt; r0 += 28) {
            const int r = r0 + sub;
            const bool in = lane < 63 && r < cnt;
            const float v = in ? s_acc[r * SV + col] : 0.0f;
            const unsigned long long nz = ballot(v != 0.0f);
            const bool any = in && ((nz >> (sub * SV)) & 0x1ffull) != 0;   // rows of zeros stay untouched
            GS_STAT(11, __popcll(ballot(any && col == 0)));   // flushed rows
            if (any) {
                const int g = s_idx[r];
                float* dst;
                if (slab) dst = g_rgb + (size_t)g * SV + col;   // [V, 9]: rgb 3 | opacity 1 | uv 2 | conic 3
                else if (col < 3) dst = g_rgb + (size_t)g * 3 + col;
                else if (col == 3) dst = g_opa + g;
                else if (col < 6) dst = g_uv + (size_t)g * 2 + (col - 4);
                else dst = g_conic + (size_t)g * 3 + (col - 6);
                global_add(dst, v);
            }
        }
        GS_PHASE(4);
    }
    GS_STAT_FLUSH(16);
