// forward.hip — das3r_raster_forward as a ForwardCall with named steps, and the host state only a forward touches: the per-thread
// PerDevice record with its mailbox (protocol: mailbox.h) and rings, the per-stream side streams and depth-histogram slots, the join of
// the split preprocess.  Host code only: this file defines no kernel.  The decisions are made elsewhere — which binning path and whether to
// speculate: path_policy.h; which compositing kernel: kernel_choice.h; the buffer layout: api.hip compute_layout.
#include <string.h>

#include <algorithm>
#include <vector>

#include "host_state.h"

namespace das3r {

// The split preprocess (preprocess.hip: geometry kernel on the caller's stream, SH colour kernel on a side stream beside the binning chain):
// taken or not from the call's SHAPE alone, never from a timing, so that a job computes with the same kernels however it was scheduled (both
// forms store the same bits; the rule keeps the launch sequence reproducible too).
//   binning_path   0 the global depth sort (it scatters the depth keys the colour kernel reads: fused kernel)
//                  1 index-order emission with a binning chain of its own (local order, segmented): the window the colour kernel fills
//                  2 emission fused into the preprocess kernel (P <= 196 k, the whole grid resident: no chain to run beside)
//   forced         Switches::split_colour: -1 never, 1 wherever it can run (SH given, active degree >= 1, path 1), 0 by shape:
// active degree >= 2 (rows of 108 / 192 bytes and the nine Jacobian planes: at degree 0 / 1 the colour is 12 / 48 bytes of input, nothing to
// hide), P >= SPLIT_MIN_P (below that the colour kernel is a few microseconds, of the order of the fork and the join themselves), and a
// forward a backward may follow (flags bit 3 clear on the way in).  An evaluation forward keeps the fused kernel: its callers wait for every
// view, and where the stream has run dry before the call — the no-grad glue render, bench.py's eval_forward — the six host calls of the fork
// and the join are on the critical path themselves: 3.11 -> 3.18 ms per view measured, against 0.657 -> 0.648 on the fused evaluation path.
constexpr int SPLIT_MIN_P = 1 << 18;
bool split_colour_rule(bool has_sh, int sh_degree, int P, int binning_path, bool no_backward, int forced) {
    if (!has_sh || sh_degree < 1 || binning_path != 1 || forced < 0 || P <= 0) return false;
    if (forced > 0) return true;
    return sh_degree >= 2 && P >= SPLIT_MIN_P && !no_backward;
}

// What the library keeps per (host thread, device, caller stream), created at the stream's first forward that needs it:
//   * one side stream and its two events, from the first split forward of the stream on.  K jobs in flight (farm.run_jobs: K host
//     threads, each on its own stream) get one each; the hardware queue count is the runtime's business.  (A side stream of the lowest
//     priority the device offers measured the same as this one: ledger.)  Destroyed with the thread.
//   * the depth histograms of the segmented path (segkey.h), round 6: two 256-word slots, used in turn.  A forward's preprocess kernel
//     accumulates into one and ZEROES THE OTHER for the next forward of the stream — the memset that used to precede every forward (a launch
//     of its own: 5 us of every DAS3R-shaped iteration) is gone.  Launches of one stream are ordered, so the slot a forward zeroes is read by
//     nobody (the previous forward's emission has finished), and the slot it reads stays as it is until the NEXT forward's preprocess kernel,
//     however often its own emission is redone.  Should a slot ever be dirty — an aborted forward — the buckets come out less even for one
//     forward and exact all the same: any histogram gives a monotone map, the same one in every workgroup.  NOT freed with the thread:
//     hipFree synchronises the device, and other threads may be rendering.
struct PerStream {
    int dev;
    hipStream_t caller;
    SideStream side = {nullptr, nullptr, nullptr, 0};   // side.stream == null: none yet
    uint32_t *dhist = nullptr;                          // null: none yet
    uint32_t turn = 0;
};
struct PerStreams {
    std::vector<PerStream> all;
    ~PerStreams() {
        for (auto &e : all) {
            if (!e.side.stream) continue;
            (void)hipEventDestroy(e.side.fork);
            (void)hipEventDestroy(e.side.join);
            (void)hipStreamDestroy(e.side.stream);
        }
    }
};
static int per_stream(hipStream_t s, PerStream **out) {   // (*out is good until this thread's next call of per_stream)
    static thread_local PerStreams streams;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    for (auto &e : streams.all)
        if (e.dev == dev && e.caller == s) { *out = &e; return DAS3R_OK; }
    streams.all.push_back(PerStream{dev, s});
    *out = &streams.all.back();
    return DAS3R_OK;
}
static int side_stream_for(hipStream_t s, SideStream *out) {
    PerStream *e = nullptr;
    const int r = per_stream(s, &e);
    if (r) return r;
    if (!e->side.stream) {
        SideStream ss = {nullptr, nullptr, nullptr, 0};
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->dev));
        ss.colour_blocks = COLOUR_WGS_PER_CU * (cus > 0 ? cus : 1);
        HIP_TRY(hipStreamCreateWithFlags(&ss.stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ss.join, hipEventDisableTiming));
        e->side = ss;
    }
    *out = e->side;
    return DAS3R_OK;
}
static bool dhist_slots(hipStream_t s, uint32_t **use, uint32_t **next) {
    PerStream *e = nullptr;
    if (per_stream(s, &e)) return false;
    if (!e->dhist) {
        uint32_t *buf = nullptr;
        if (hipMalloc((void **)&buf, 2 * 256 * sizeof(uint32_t)) != hipSuccess) return false;
        if (hipMemsetAsync(buf, 0, 2 * 256 * sizeof(uint32_t), s) != hipSuccess) return false;   // (on the stream whose kernels use it: ordered)
        e->dhist = buf;
    }
    e->turn++;
    *use = e->dhist + 256 * (e->turn & 1u);
    *next = e->dhist + 256 * ((e->turn + 1u) & 1u);
    return true;
}
// The depth histogram of this forward (segkey.h): filled by the preprocess kernel, read by the emission.  Not segmented: none (nulls).
// No slot: in the geometry buffer, zeroed by a memset, as before round 6 (*next stays null).
static int seg_dhist_for(bool seg, hipStream_t s, const Buffers &v, uint32_t **use, uint32_t **next) {
    *use = *next = nullptr;
    if (seg && !dhist_slots(s, use, next)) {
        *use = v.g_dhist();
        HIP_TRY(hipMemsetAsync(*use, 0, 4 * 256, s));
    }
    return DAS3R_OK;
}

int validate(const das3r_raster_args *a, const das3r_raster_in *in) {
    if (!a || !in) { set_error("null args"); return DAS3R_ERR_INVALID_ARG; }
    if (a->P < 0 || a->image_width <= 0 || a->image_height <= 0) { set_error("bad extents P=%d W=%d H=%d", a->P, a->image_width, a->image_height); return DAS3R_ERR_INVALID_ARG; }
    if ((int64_t)((a->image_width + TILE_X - 1) / TILE_X) * ((a->image_height + TILE_Y - 1) / TILE_Y) >= (1ll << 22)) {   // render_common.h pack_tiles
        set_error("image of %d x %d pixels has 2^22 tiles or more", a->image_width, a->image_height);
        return DAS3R_ERR_INVALID_ARG;
    }
    if (a->P == 0) return DAS3R_OK;
    if (!a->bg || !a->viewmatrix || !a->projmatrix || !a->campos) { set_error("bg/viewmatrix/projmatrix/campos must be device pointers"); return DAS3R_ERR_INVALID_ARG; }
    if (in->pre) {   // ABI 14: raw parameters + pose; the camera-frame tensors are not looked at
        const das3r_pretransform *p = in->pre;
        if (!p->xyz || !p->rot || !p->scaling || !p->opacity_raw || !p->conf_flat || !p->R || !p->t || !p->Lq) { set_error("das3r_raster_in.pre: xyz / rot / scaling / opacity_raw / conf_flat / R / t / Lq are required"); return DAS3R_ERR_INVALID_ARG; }
        if (in->cov3D_precomp) { set_error("das3r_raster_in.pre excludes cov3D_precomp"); return DAS3R_ERR_INVALID_ARG; }
    } else if (!in->means3D || !in->opacities) { set_error("means3D/opacities are required"); return DAS3R_ERR_INVALID_ARG; }
    if ((in->shs != nullptr) == (in->colors_precomp != nullptr)) { set_error("Please provide excatly one of either SHs or precomputed colors!"); return DAS3R_ERR_INVALID_ARG; }
    const bool sr = in->pre != nullptr || (in->scales != nullptr && in->rotations != nullptr);
    if ((!in->pre && (in->scales != nullptr) != (in->rotations != nullptr)) || sr == (in->cov3D_precomp != nullptr)) {
        set_error("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
        return DAS3R_ERR_INVALID_ARG;
    }
    if (in->shs) {
        if (a->sh_degree < 0 || a->sh_degree > 3) { set_error("sh_degree must be 0..3 (got %d)", a->sh_degree); return DAS3R_ERR_INVALID_ARG; }
        if (a->M < (a->sh_degree + 1) * (a->sh_degree + 1) || a->M > 16) { set_error("M=%d incompatible with sh_degree=%d (need (D+1)^2 <= M <= 16)", a->M, a->sh_degree); return DAS3R_ERR_INVALID_ARG; }
    }
    if (a->tanfovx <= 0.f || a->tanfovy <= 0.f) { set_error("tanfov must be positive"); return DAS3R_ERR_INVALID_ARG; }
    return DAS3R_OK;
}

int per_device(PerDevice **out) {
    static thread_local PerDevice state[MAX_DEVICES];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) { set_error("device ordinal %d not supported", dev); return DAS3R_ERR_INVALID_ARG; }
    PerDevice &T = state[dev];
    register_rendering_thread(dev);   // (grid_is_resident: a second rendering thread on the device switches the ticket-free short cut off)
    if (!T.mb.host) {
        uint32_t *h = nullptr;
        HIP_TRY(hipHostMalloc((void **)&h, MAILBOX_BYTES, hipHostMallocMapped));
        memset(h, 0, MAILBOX_BYTES);
        HIP_TRY(hipHostGetDevicePointer((void **)&T.mb.dev, h, 0));
        T.mb.host = h;
    }
    *out = &T;
    return DAS3R_OK;
}
// spin until `*word` carries `tag` — bounded: a look at the stream now and then, at last a stream synchronise and one more look.
// *seen = what the word held at that last look (the caller decides what a missing tag means)
static int await_tag(volatile uint32_t *word, uint32_t tag, hipStream_t s, uint32_t *seen) {
    for (long spins = 0; spins < 200000000L; spins++) {
        if ((*seen = __atomic_load_n(word, __ATOMIC_ACQUIRE)) == tag) return DAS3R_OK;
        __builtin_ia32_pause();
        if ((spins & 0xFFFFF) == 0xFFFFF && hipStreamQuery(s) != hipErrorNotReady) break;   // stream drained (or failed): stop spinning
    }
    HIP_TRY(hipStreamSynchronize(s));
    *seen = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    return DAS3R_OK;
}
// wait for word `idx` to carry `tag`, or give up loudly
static int mailbox_wait(Mailbox *mb, int idx, uint32_t tag, hipStream_t s) {
    uint32_t seen = 0;
    const int r = await_tag(&mb->host[idx], tag, s, &seen);
    if (r) return r;
    if (seen == tag) return DAS3R_OK;
    set_error("the device never delivered the result of this forward to the host mailbox");
    return DAS3R_ERR_HIP;
}

// Examine the self-check word a forward's last binning kernel left in `slot` (mailbox.h examine_check_word says what is in it and what
// comes back; the waiting is await_tag on `s`).  Returns 1 when the slot does not hold `tag`'s word.
static unsigned long long g_stats[4] = {0, 0, 0, 0};   // forwards, self-check words examined, rescued look-back polls, failed self-checks
static void stat_add(int i) { __atomic_fetch_add(&g_stats[i], 1ull, __ATOMIC_RELAXED); }
int examine_check_slot(volatile uint32_t *slot, uint32_t tag, bool wait, hipStream_t s) {
    const CheckResult c = examine_check_word(slot, tag, wait, [s](volatile uint32_t *word, uint32_t t, uint32_t *seen) { return await_tag(word, t, s, seen); });
    if (c.error) return c.error;
    if (c.state == CHECK_NOT_THERE) return 1;
    for (int i = 1; i < 4; i++)
        if (c.stats >> i & 1u) stat_add(i);
    if (c.rescued && switches().verbose) fprintf(stderr, "das3r: a look-back poll needed the read-modify-write path\n");
    if (c.state != CHECK_FAILED) return DAS3R_OK;
    set_error("a forward's binning failed its self-check (flags 0x%x); its output is invalid", c.flags);
    return DAS3R_ERR_HIP;
}
// how a thread's CheckSlots (mailbox.h) examine slot i of its mailbox
struct SlotExaminer {
    Mailbox *mb;
    hipStream_t s;
    int operator()(uint32_t i, uint32_t tag, bool wait) const { return examine_check_slot(mb->host + check_word_index(i), tag, wait, s); }
};

// per call: top word + 64 sub-counters, one 64-byte line each; the emission ring has as many slots, each {err + padding, ghist, status granules}
constexpr uint32_t ARRIVE_SLOTS = 16, ARRIVE_WORDS = 8 + 64 * 8;
constexpr size_t EMIT_SLOT_BYTES = sizeof(uint32_t) * EMIT_SLOT_WORDS + sizeof(unsigned long long) * EMIT_STATUS_GRANULES;

// The split preprocess: the fork event is recorded behind the geometry kernel (launch_preprocess); the colour kernel goes to the side
// stream once the binning kernels are enqueued on s (ForwardCall::colour_launch), and s waits for it (colour_join) in front of the first
// kernel that reads a colour, `clamped` or a Jacobian plane — the compositing forward.  Whatever is pending on the side stream when the
// call returns, on EVERY way out, s waits for (the destructor): once the call's work on s is complete the side stream touches neither the
// caller's tensors nor the geometry buffer.  (A way out between the fork and the launch leaves nothing on the side stream.)
struct Join {
    hipStream_t s;
    SideStream side = {nullptr, nullptr, nullptr, 0};
    bool forked = false, pending = false;
    ~Join() {
        if (pending) (void)hipStreamWaitEvent(s, side.join, 0);
    }
};

// One das3r_raster_forward call.  Host <-> device hand-offs of one forward (all through the pinned mailbox, no copies, no events):
//   * num_rendered (sum of tiles_touched) leaves with the preprocess kernel, five kernels before the device needs it, so
//     the binning buffer is sized exactly and the host practically never waits (upstream blocks on a cudaMemcpy in the
//     middle of every forward); on the local-order path nothing waits for it at all (speculative capacity, below);
//   * the binning self-check word is delivered by the last binning kernel into a slot of the mailbox; saved->check_word /
//     check_tag name it.  It is examined by das3r_raster_backward (before anything is launched) and das3r_raster_check, which
//     wait for it, and — for callers that use neither — without waiting at the start of this thread's later forwards;
//     debug mode waits for it before returning.
struct ForwardCall {
    const das3r_raster_args *a;
    const das3r_raster_in *in;
    const das3r_raster_out *out;
    das3r_alloc_fn alloc_geom, alloc_binning, alloc_img;
    void *user;
    das3r_raster_saved *saved;
    hipStream_t s;
    Join join;                             // (s again: what the side stream owes the caller's)
    PerDevice *T = nullptr;
    Mailbox *mb = nullptr;
    Buffers v{};                           // saved's three buffers, laid out for v.L.capacity instances; layout_and_alloc is the one place that changes the layout
    PolicyInputs policy_in;
    ForwardPlan plan;
    bool local = false;                    // plan.local, until the exact flow's count says "global sort after all"
    bool shjac = false, depth = false, no_backward = false, aa = false;
    uint32_t count_tag = 0, late_tag = 0;
    const uint32_t *seg_dhist = nullptr;   // where this forward's depth histogram is (set with the preprocess launch)
    unsigned long long *arrive = nullptr;  // this call's arrival words

    int64_t run();
    int check_arguments();
    int empty_scene();
    int arrival_ring();
    int layout_and_alloc(int64_t cap);
    int preprocess(int binning_path, const EmitArgs *emit);
    int colour_launch();
    int colour_join();
    int claim_check_slot(uint32_t **host_late);
    int look_at_lists(LocalBin *lb);
    int bin_and_render(bool local_order, bool ctrl_zeroed, uint32_t *count_out = nullptr, uint32_t count_out_tag = 0, uint32_t *emit_slot = nullptr);
    int read_count(int64_t *I);
    int flow_fused_emit(int64_t *I);
    int flow_speculative(int64_t *I);
    int after_speculation(int64_t *I);
    int flow_exact(int64_t *I);
    int redo_exact(int64_t I);
};

int ForwardCall::check_arguments() {
    const int rc = validate(a, in);
    if (rc) return rc;
    if (!out || !out->out_color || (a->P > 0 && !out->radii) || !alloc_geom || !alloc_binning || !alloc_img || !saved) {
        set_error("das3r_raster_forward: null output/allocator");
        return DAS3R_ERR_INVALID_ARG;
    }
    if (out->out_invdepth && !fwd_has_invdepth_form(switches().render_fwd)) {   // ABI 16: every forward kernel the library picks has an inverse-depth form, not the forced slices
        set_error("das3r_raster_forward: DAS3R_RENDER=%s has no inverse-depth form (das3r_raster_out.out_invdepth)", fwd_kernel_name(switches().render_fwd));
        return DAS3R_ERR_INVALID_ARG;
    }
    return DAS3R_OK;
}

int64_t ForwardCall::run() {
    int rc = check_arguments();
    if (rc) return rc;
    stat_add(0);   // (a refused call is no forward: das3r_get_stats is unchanged by it, tests/test_gpu_tile_grids.py)
    const int P = a->P, W = a->image_width, H = a->image_height;
    depth = out->out_invdepth != nullptr;   // ABI 16: the binning buffer also holds Layout::d_* (d_bytes instead of binning_bytes)
    // the geometry buffer also holds Layout::g_shjac (flags bit 2) — unless the caller said that no backward will read it (flags bit 3 on the
    // way in, read before the struct is cleared below)
    shjac = in->shs != nullptr && a->sh_degree >= 2 && !(saved->flags & NO_BACKWARD_IN_FLAG);
    no_backward = (saved->flags & NO_BACKWARD_IN_FLAG) != 0;
    aa = (saved->flags & ANTIALIAS_FLAG) != 0;   // (bit 4 on the way in: an antialiased forward; set again on the way out)
    compute_layout(P, 0, W, H, &v.L, shjac);
    saved->geom = v.geom = v.recs = alloc_geom(user, v.L.pub.geom_bytes);
    saved->img = v.img = alloc_img(user, v.L.pub.img_bytes);
    saved->binning = v.binning = nullptr;
    saved->num_rendered = 0;
    saved->capacity = 0;
    saved->check_word = nullptr;
    saved->check_tag = 0;
    saved->flags = aa ? ANTIALIAS_FLAG : 0u;
    if (!saved->geom || !saved->img) { set_error("scratch allocation failed (geom %zu B, img %zu B)", v.L.pub.geom_bytes, v.L.pub.img_bytes); return DAS3R_ERR_ALLOC; }
    if (P == 0) return empty_scene();
    if ((rc = per_device(&T))) return rc;
    mb = &T->mb;
    if ((rc = T->checks.settle_all(SlotExaminer{mb, s}))) return rc;
    if ((rc = arrival_ring())) return rc;
    // Which binning path this forward takes, whether it speculates on its capacity and whether it looks at its tile lists: path_policy.h,
    // from what the earlier forwards of the shape left in T->verdict and the two words their kernels may have raised since (kept as found:
    // the words are cleared when read — a forward that fails further down has still consumed them).
    const uint32_t too_long = mb->host[MB_TOO_LONG];
    if (too_long) mb->host[MB_TOO_LONG] = 0;
    const uint32_t want_bits = mb->host[MB_WANT_BITS];
    if (want_bits) mb->host[MB_WANT_BITS] = 0;
    policy_in = PolicyInputs{P, W, H, v.L.ntiles, v.L.tbits, v.L.tile_passes, too_long, want_bits, switches().binning /* DAS3R_BINNING */, use_onesweep(),
                             a->capacity_hint, switches().capacity_exact, &T->resume};
    plan = plan_forward(T->verdict, policy_in);
    local = plan.local;
    count_tag = next_tag(mb);
    arrive = T->arrive_ring + (size_t)(count_tag % ARRIVE_SLOTS) * ARRIVE_WORDS;
    int64_t I = 0;
    // The speculative flows: the binning buffer is laid out for the plan's capacity and the whole forward is enqueued before the host looks
    // at the mailbox (the kernels clamp to the capacity).  Should the scene have grown past it, the binning and the compositing are redone
    // with the exact size.  The count is not needed before the end of this call: the preprocess kernel skips its count reduction and the
    // scan delivers it.  When the preprocess grid is resident as a whole (P <= 196 k) the scan and the emission run inside the preprocess
    // kernel itself (EmitArgs, common.h) and the separate scan + emit kernel is not launched at all.  DAS3R_FUSED_EMIT=0 switches that off.
    if (plan.speculate) {
        if ((rc = layout_and_alloc(plan.cap))) return rc;
        const bool fused_emit = local && grid_is_resident(div_up(P, 256)) && !switches().fused_emit_off;
        rc = fused_emit ? flow_fused_emit(&I) : flow_speculative(&I);
    } else {
        rc = flow_exact(&I);
    }
    if (rc) return rc;
    if (a->debug && late_tag && (rc = T->checks.settle(check_slot_of(late_tag), true, SlotExaminer{mb, s}))) return rc;   // debug: report this forward's self-check word right away
    saved->num_rendered = I;
    saved->capacity = v.L.capacity;
    if (depth) saved->flags |= DEPTH_SAVED_FLAG;
    if (shjac) saved->flags |= SHJAC_SAVED_FLAG;
    return I;
}

// upstream:rasterize_points.cu skips the rasterizer when P == 0: the image stays zero (background NOT applied)
int ForwardCall::empty_scene() {
    const int W = a->image_width, H = a->image_height;
    HIP_TRY(hipMemsetAsync(out->out_color, 0, sizeof(float) * 3 * (size_t)W * H, s));
    if (out->out_invdepth) HIP_TRY(hipMemsetAsync(out->out_invdepth, 0, sizeof(float) * (size_t)W * H, s));
    HIP_TRY(hipMemsetAsync(v.ranges(), 0, 8 * (size_t)v.L.ntiles, s));
    saved->binning = alloc_binning(user, 256);   // (kept as found: 256 bytes nobody reads, and no look at what the allocator returned)
    return 0;
}

// per-thread ring of self re-arming arrival words for the count reduction of the preprocess kernel
int ForwardCall::arrival_ring() {
    if (T->arrive_ring) return DAS3R_OK;
    HIP_TRY(hipMalloc((void **)&T->arrive_ring, ARRIVE_SLOTS * ARRIVE_WORDS * sizeof(unsigned long long)));
    // on the CALLER'S stream, in front of the kernel that counts in it: hipMemset runs on the null stream, which a non-blocking stream
    // does not wait for — with a second job keeping the GPU busy (round 5: farm.run_jobs) the fill could land AFTER the first preprocess
    // kernel of this thread had started counting, the last arriver never saw its total, and the forward ended with "the device never
    // delivered the result of this forward to the host mailbox" (one first-forward in a few dozen two-job runs)
    HIP_TRY(hipMemsetAsync(T->arrive_ring, 0, ARRIVE_SLOTS * ARRIVE_WORDS * sizeof(unsigned long long), s));
    // ... and COMPLETE before this call goes on: the ring belongs to the thread, not to the stream — the same thread's next forward may
    // be issued on another non-blocking stream, which does not wait for this one.  Once per thread and device (kept as found).
    HIP_TRY(hipStreamSynchronize(s));
    return DAS3R_OK;
}

// Lay L out for `cap` instances — with the plan's depth buckets when it is segmented (compute_layout starts every layout without) — and
// have the caller allocate the binning buffer.
int ForwardCall::layout_and_alloc(int64_t cap) {
    compute_layout(a->P, cap, a->image_width, a->image_height, &v.L, shjac);
    v.L.dhist_ptr = seg_dhist;
    if (plan.seg) {
        v.L.dbits = plan.seg_bits;
        v.L.kbits = v.L.tbits + plan.seg_bits;
        v.L.kshift = std::min(16, 32 - v.L.kbits);
        v.L.part_passes = plan.seg_passes;
    }
    saved->binning = v.binning = alloc_binning(user, depth ? v.L.d_bytes : v.L.pub.binning_bytes);
    if (saved->binning) return DAS3R_OK;
    set_error("scratch allocation failed (binning %zu B)", v.L.pub.binning_bytes);   // (kept as found: binning_bytes even for a depth forward, which asked for d_bytes)
    return DAS3R_ERR_ALLOC;
}

// The preprocess kernel, on binning path 0 / 1 / 2 (split_colour_rule).  emit: the emission fused in (path 2) — no depth histogram then.
// A speculative forward has its binning buffer already: the kernel zeroes its control words and skips the count reduction (no arrival words).
int ForwardCall::preprocess(int binning_path, const EmitArgs *emit) {
    int rc;
    uint32_t *dhist = nullptr, *dhist_next = nullptr;
    if (!emit && (rc = seg_dhist_for(plan.seg, s, v, &dhist, &dhist_next))) return rc;
    v.L.dhist_ptr = seg_dhist = dhist;   // (the emission reads it; a layout made later takes it from seg_dhist)
    const SideStream *side = nullptr;   // null = the fused kernel
    if (split_colour_rule(in->shs != nullptr, a->sh_degree, a->P, binning_path, no_backward, switches().split_colour)) {
        if ((rc = side_stream_for(s, &join.side))) return rc;
        side = &join.side;
    }
    if ((rc = launch_preprocess(a, in, out->radii, v, plan.speculate ? v.b_ctrl() : WordRange{nullptr, 0}, plan.speculate ? nullptr : arrive, mb->dev, count_tag, s,
                                emit, dhist, dhist_next, aa, side))) return rc;
    join.forked = side != nullptr;
    return DAS3R_OK;
}

int ForwardCall::colour_launch() {
    if (!join.forked) return DAS3R_OK;
    join.forked = false;
    join.pending = true;   // (from the first call that touches the side stream on)
    return launch_sh_colour(a, in, v, &join.side);
}
int ForwardCall::colour_join() {
    const int r = colour_launch();
    if (r) return r;
    if (!join.pending) return DAS3R_OK;
    join.pending = false;
    HIP_TRY(hipStreamWaitEvent(s, join.side.join, 0));
    return DAS3R_OK;
}

// this forward's self-check word: a tag and a slot of its own (after the forward that used the slot CHECK_SLOTS forwards ago)
int ForwardCall::claim_check_slot(uint32_t **host_late) {
    late_tag = next_tag(mb);
    uint32_t slot = 0;
    const int r = T->checks.claim(late_tag, &slot, SlotExaminer{mb, s});
    if (r) return r;
    *host_late = mb->dev + check_word_index(slot);
    saved->check_word = (void *)(mb->host + check_word_index(slot));
    saved->check_tag = late_tag;
    return DAS3R_OK;
}

// The three questions — look at the list skew? order the tiles longest first? leave the backward its hint? — are asked with
// local_lists = false, "by shape", on every binning path: lb->point_list is only set afterwards, so that is what these sites have always
// answered.  launch_render_forward, which sees the pointer, passes the truth, and on the local-order path never takes the lanes /
// regions kernels the answers here are about; the hint's bit 0 still steers that forward's BACKWARD (kernel_choice.h choose_backward).
// Kept as it is: changing it changes which kernels a training run takes.
int ForwardCall::look_at_lists(LocalBin *lb) {
    int r;
    const int P = a->P;
    const int64_t cap = v.L.capacity;
    const bool by_shape = cap > 0 && quad_lanes(switches(), v.L.ntiles, v.L.capacity, /*local_lists=*/false);
    if (plan.decide_fine && by_shape) {   // (shapes the one-workgroup-per-tile kernel would take: few tiles, long lists)
        const uint32_t tag = next_tag(mb);
        if ((r = launch_list_skew(v, (uint32_t)cap, (uint32_t)(P - 1), mb->dev + MB_LONGEST, tag, a->debug != 0, s))) return r;
        if ((r = mailbox_wait(mb, MB_SKEW_TAG, tag, s))) return r;
        const uint32_t longest = mb->host[MB_LONGEST], crowd16 = mb->host[MB_CROWD16];
        const int64_t mean = skew_mean(T->verdict, cap, v.L.ntiles);
        const bool now_fine = learn_skew(T->verdict, longest, crowd16, cap, v.L.ntiles);
        if (switches().verbose) fprintf(stderr, "[das3r] tile lists: longest %lld, mean %lld, %.1f of 64 consecutive entries in one quadrant -> %s kernels\n", (long long)longest,
                                        (long long)mean, crowd16 / 16.0, now_fine ? "2x2-region" : "block");
    }
    const bool fine = prefers_regions(T->verdict);
    lb->prefer_regions = fine;
    lb->tile_order = nullptr;
    if (tile_lpt_wanted(switches(), v.L.ntiles, v.L.capacity, /*local_lists=*/false, fine)) {   // longest lists first (kernel_choice.h says why)
        if ((r = launch_tile_lpt(v, (uint32_t)cap, a->debug != 0, s))) return r;
        lb->tile_order = v.i_order();
    }
    if (fine && by_shape) saved->flags |= backward_hint(T->verdict, (uint32_t)BUCKET);   // (for the backward pass of this forward: kernel_choice.h choose_backward)
    return DAS3R_OK;
}

// everything behind the count: scan + emission, partition, tile ranges, compositing (L laid out for its capacity, buffer allocated)
// emit_slot: the preprocess kernel has emitted the instances already
int ForwardCall::bin_and_render(bool local_order, bool ctrl_zeroed, uint32_t *count_out, uint32_t count_out_tag, uint32_t *emit_slot) {
    int r;
    const int P = a->P;
    const int64_t cap = v.L.capacity;
    const bool fused_scan = use_onesweep();   // scan + emission in one kernel; the classic path scans, then emits
    const bool seg = v.L.dbits > 0;           // segmented path: index-order emission with depth buckets, lists sorted by segment_sort_kernel
    const bool finish = seg && plan.bucket_local;   // ... or, with the same emission and passes, finished by the compositing kernel (path_policy.h bucket_local_rule)
    // (plan.cells, with finish: launch_binning's partition step is launch_cell_sort — partition by reserved ranges + finish per cell, which
    //  writes the tile ranges and hands over the self-check word — instead of the stable passes and tile_ranges_kernel: cells_rule)
    if (!emit_slot) {
        if (fused_scan) {
            if ((r = launch_binning_scan_emit(P, cap, out->radii, v, ctrl_zeroed, count_out, count_out_tag, a->debug != 0,
                                              s, local_order || seg))) return r;
        } else if ((r = launch_scan(P, v, nullptr, 0, a->debug != 0, s))) return r;
    }
    uint32_t *host_late = nullptr;
    if (cap > 0 && (r = claim_check_slot(&host_late))) return r;
    uint32_t *dead_keys = nullptr;
    if ((r = launch_binning(P, cap, a->image_width, a->image_height, out->radii, v, fused_scan, host_late, late_tag,
                            a->debug != 0, s, &dead_keys, emit_slot, mb->dev + MB_TOO_LONG, plan.gen, finish, finish && plan.cells))) return r;
    if ((r = colour_launch())) return r;   // the split preprocess: the colour kernel, beside the binning kernels enqueued above
    LocalBin lb = {v.b_ckpt(), nullptr, nullptr, nullptr, nullptr, plan.gen, (uint32_t)(P - 1), (uint32_t)cap};
    if ((r = look_at_lists(&lb))) return r;
    if ((local_order || finish) && cap > 0) {
        lb.point_list = v.point_list();
        lb.slot_list = v.b_slot();
        lb.keys = dead_keys;   // (finish: the bucketed keys of the last pass, read before a list too long for LDS takes its own stretch as scratch)
        lb.host_flag = mb->dev + MB_TOO_LONG;
        if (finish) lb.dbits = v.L.dbits, lb.fbits = v.L.kshift;
    }
    if ((r = colour_join())) return r;   // (a redo finds the colours there already: nothing is pending the second time)
    return launch_render_forward(a, in->colors_precomp, out->out_color, v, lb, s, out->out_invdepth, depth ? v.d_ckpt() : nullptr);
}

// Wait for this forward's count (usually there already).  prefiltered: the caller's promise that no point fails the near-plane cull
// (upstream traps when one does: auxiliary.h in_frustum); the preprocess kernel leaves this call's tag in mailbox word 12 when one did.
int ForwardCall::read_count(int64_t *I) {
    const int rc = mailbox_wait(mb, MB_COUNT_TAG, count_tag, s);
    if (rc) return rc;
    if (a->prefiltered && mb->host[MB_FILTERED] == count_tag) {
        set_error("Point is filtered although prefiltered is set. This shouldn't happen!");
        return DAS3R_ERR_INVALID_ARG;
    }
    *I = (int64_t)mb->host[MB_COUNT];
    if (*I > CAPACITY_MAX) { set_error("num_rendered %lld exceeds 2^31", (long long)*I); return DAS3R_ERR_OVERFLOW; }
    return DAS3R_OK;
}

// Speculative, the scan and the emission inside the preprocess kernel: their control words live in a library-owned ring slot per forward,
// zero at rest (mailbox.h EmitRingState says when the ring is zeroed again).
int ForwardCall::flow_fused_emit(int64_t *I) {
    int rc;
    if (!T->emit_ring) HIP_TRY(hipMalloc((void **)&T->emit_ring, ARRIVE_SLOTS * EMIT_SLOT_BYTES));
    if (T->emit.wants_zeroing(count_tag)) {   // first use, an aborted forward, or the tags wrapped around
        HIP_TRY(hipMemsetAsync(T->emit_ring, 0, ARRIVE_SLOTS * EMIT_SLOT_BYTES, s));
        T->emit.zeroed();
    }
    uint32_t *emit_slot = (uint32_t *)(T->emit_ring + (size_t)(count_tag % ARRIVE_SLOTS) * EMIT_SLOT_BYTES);
    const EmitArgs em = {(unsigned long long *)(emit_slot + EMIT_SLOT_WORDS), count_tag, emit_slot + 64, emit_slot,
                         v.b_keyA(), v.b_gid_of(), v.g_off_by_gid(), (uint32_t)v.L.capacity, v.L.tbits, v.g_count(), mb->dev};
    T->emit.taken_by(count_tag);   // (kept as found: marked dirty before launch_preprocess, clean again only after bin_and_render returned 0)
    if ((rc = preprocess(2, &em))) return rc;
    if ((rc = bin_and_render(true, true, nullptr, 0, emit_slot))) return rc;
    T->emit.rearmed();
    return after_speculation(I);
}

// Speculative, with the scan + emit kernel, which delivers the count.
int ForwardCall::flow_speculative(int64_t *I) {
    int rc;
    if ((rc = preprocess(1, nullptr))) return rc;
    if ((rc = bin_and_render(local, true, mb->dev, count_tag))) return rc;
    return after_speculation(I);
}

int ForwardCall::after_speculation(int64_t *I) {
    const int rc = read_count(I);
    if (rc) return rc;
    (void)learn_count(T->verdict, *I, policy_in, plan);   // (kept as found: the result is ignored — enqueued already, this forward keeps its path)
    return *I > v.L.capacity ? redo_exact(*I) : DAS3R_OK;
}

// The scene outgrew the speculative capacity: binning and compositing again, laid out for exactly I.
int ForwardCall::redo_exact(int64_t I) {
    const int rc = layout_and_alloc(I);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(v.g_ctrl().begin, 0, v.g_ctrl().bytes, s));   // tickets and look-back words of the scan
    HIP_TRY(hipMemsetAsync(v.ranges(), 0, 8 * (size_t)v.L.ntiles, s));
    return bin_and_render(local, false);
}

// Exact: the preprocess kernel counts, the host waits for the count (usually there already: preprocess finished long ago) and sizes the
// binning buffer for it.
int ForwardCall::flow_exact(int64_t *I) {
    int rc;
    const int P = a->P;
    const bool seg = plan.seg, debug = a->debug != 0;
    if ((rc = preprocess((local || seg) ? 1 : 0, nullptr))) return rc;
    if (!local && !seg && (rc = launch_depth_sort(P, v, 0, WordRange{nullptr, 0}, debug, s))) return rc;
    if ((rc = read_count(I))) return rc;
    if (learn_count(T->verdict, *I, policy_in, plan)) {   // the scene grew: global sort after all
        local = false;
        if ((rc = colour_join())) return rc;   // (the sort scatters the depth keys the colour kernel reads)
        // (kept as found: part 0 runs here whenever the count says so, after the join — also when it ran above, also on the segmented path)
        if ((rc = launch_depth_sort(P, v, 0, WordRange{nullptr, 0}, debug, s))) return rc;
    }
    if ((rc = layout_and_alloc(*I))) return rc;
    if (!local && !seg && (rc = launch_depth_sort(P, v, 1, v.b_ctrl(), debug, s))) return rc;
    return bin_and_render(local, !local && !seg);
}

}  // namespace das3r

using namespace das3r;

// The self-check of the forward that produced `saved`, for callers that want it BEFORE they consume the image (the forward
// itself returns as soon as everything is enqueued; das3r_raster_backward runs this first).  Waits, bounded, for the word.
extern "C" int das3r_raster_check(const das3r_raster_saved *saved, das3r_stream_t stream) {
    if (!saved) { set_error("das3r_raster_check: null saved state"); return DAS3R_ERR_INVALID_ARG; }
    if (!saved->check_word || !saved->check_tag) return DAS3R_OK;   // P == 0, nothing rendered, or a caller that dropped the ticket
    const int r = examine_check_slot((volatile uint32_t *)saved->check_word, saved->check_tag, true, (hipStream_t)stream);
    return r < 0 ? r : DAS3R_OK;
}

extern "C" void das3r_get_stats(uint64_t out[4]) {
    for (int i = 0; i < 4; i++) out[i] = (uint64_t)__atomic_load_n(&g_stats[i], __ATOMIC_RELAXED);
}

extern "C" int64_t das3r_raster_forward(const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_out *out,
                                        das3r_alloc_fn alloc_geom, das3r_alloc_fn alloc_binning, das3r_alloc_fn alloc_img,
                                        void *user, das3r_raster_saved *saved, das3r_stream_t stream) {
    ForwardCall call = {a, in, out, alloc_geom, alloc_binning, alloc_img, user, saved, (hipStream_t)stream, Join{(hipStream_t)stream}};
    return call.run();
}
