// api.hip — the C-ABI entry points of libdas3r_hip.so (include/das3r_raster.h) except das3r_raster_forward / _check / das3r_get_stats
// (forward.hip), the switches, the residency rule, the profiler and the buffer layout.
#include <stdarg.h>
#include <string.h>

#include <vector>

#include "host_state.h"
#include "preprocess_choice.h"
#include <algorithm>

namespace das3r {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- per-kernel HIP-event profiler (single-threaded use: bench.py / tests) ----
struct ProfRec {
    const char *name;
    hipEvent_t start, stop;
};
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
bool profile_enabled() { return g_prof_on; }
// (events come from a pool that survives reports: creating two events per launch made the instrumented pass slower than the
//  timed one — the host fell behind the device and the gaps showed up inside the brackets: VERDICT r2 item 10)
static std::vector<hipEvent_t> g_event_pool;
static hipEvent_t pooled_event() {
    if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}
void profile_begin(const char *name, hipStream_t s) {
    ProfRec r;
    r.name = name;
    r.start = pooled_event();
    r.stop = pooled_event();
    if (!r.start || !r.stop) return;
    (void)hipEventRecord(r.start, s);
    g_prof.push_back(r);
}
void profile_end(hipStream_t s) {
    if (!g_prof.empty()) (void)hipEventRecord(g_prof.back().stop, s);
}

static Switches g_sw;
static bool g_sw_loaded = false;
static int g_inject_fault = 0;
static int g_mutate = 0;
static void load_switches() {
#ifdef DAS3R_EXPERIMENTS
    const bool experiments = true;
#else
    const bool experiments = false;
#endif
    Switches w = parse_switches(getenv, experiments);   // what every DAS3R_* spelling means: kernel_choice.h
    w.inject_fault = g_inject_fault;   // (not an environment variable: das3r_debug_inject_fault)
    w.mutate = g_mutate;               // (likewise: das3r_debug_mutate)
    g_sw = w;
    __atomic_store_n(&g_sw_loaded, true, __ATOMIC_RELEASE);
}
const Switches &switches() {
    if (!__atomic_load_n(&g_sw_loaded, __ATOMIC_ACQUIRE)) load_switches();
    return g_sw;
}

// Ticket-free chained kernels wait for lower-numbered workgroups, which is only safe while the whole grid is resident at once.
// The bound is taken from the device the call runs on (compute partitions have fewer CUs) and stays below what it holds
// (>= 3 workgroups per CU of the heaviest of these kernels).  DAS3R_TICKETS=always switches the short cut off.
// Round 6: "the whole grid is resident" presumes that the grid has the device to itself.  The library knows when it does
// not: every host thread that renders on a device registers there (forward.hip per_device(); un-registered when the thread ends), and
// once a second thread has, every chained kernel of that device takes its tickets — whatever farm.run_jobs or the environment say
// (a DAS3R_TICKETS bound set by hand still wins: it is an experiment switch, and says so once on stderr).  Two PROCESSES on one GPU
// are not seen from here: tools/jobs_per_gpu.py's process mode sets DAS3R_TICKETS=always for its children.
static int g_threads_on_device[MAX_DEVICES] = {};
struct ThreadRegistrar {
    bool on[MAX_DEVICES] = {};
    void add(int dev) {
        if (!on[dev]) { on[dev] = true; __atomic_fetch_add(&g_threads_on_device[dev], 1, __ATOMIC_RELAXED); }
    }
    ~ThreadRegistrar() {
        for (int d = 0; d < MAX_DEVICES; d++)
            if (on[d]) __atomic_fetch_sub(&g_threads_on_device[d], 1, __ATOMIC_RELAXED);
    }
};
static thread_local ThreadRegistrar g_registrar;
void register_rendering_thread(int dev) { g_registrar.add(dev); }
bool grid_is_resident(int nblocks) {
    const int forced = switches().tickets;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return false;
    const bool shared = __atomic_load_n(&g_threads_on_device[dev], __ATOMIC_RELAXED) > 1;
    if (forced >= 0) {
        static bool warned = false;
        if (shared && forced > 0 && !__atomic_exchange_n(&warned, true, __ATOMIC_RELAXED))
            fprintf(stderr, "[das3r] DAS3R_TICKETS is set to a bound while several host threads render on device %d: ticket-free chained "
                            "kernels are only safe when a grid has the device to itself\n", dev);
        return nblocks <= forced;
    }
    if (shared) return false;
    static thread_local int cached_dev = -1, cached_limit = 0;
    if (dev != cached_dev) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
        cached_dev = dev;
        cached_limit = cus * 2;   // the heaviest chained kernels get 3 workgroups per CU
    }
    return nblocks <= cached_limit;
}

int sort_ipl_override() { return switches().sort_ipl; }
#ifdef DAS3R_EXPERIMENTS
bool use_onesweep() { return !switches().sort_classic; }
#else
bool use_onesweep() { return true; }   // the three-kernel radix passes are built with EXPERIMENTS=1 only
#endif
bool use_tight_rect() { return !switches().rect_upstream; }

void compute_layout(int P, int64_t I, int W, int H, Layout *L, bool shjac) {
    memset(L, 0, sizeof(*L));
    const size_t Pn = P > 0 ? (size_t)P : 1, In = I > 0 ? (size_t)I : 1;
    L->capacity = I;
    L->tiles_x = (W + TILE_X - 1) / TILE_X;
    L->tiles_y = (H + TILE_Y - 1) / TILE_Y;
    L->ntiles = L->tiles_x * L->tiles_y;
    L->tbits = tile_bits(L->ntiles);
    L->tile_passes = (L->tbits + 7) / 8;
    L->dbits = 0;
    L->kbits = L->tbits;
    L->kshift = 0;
    L->part_passes = L->tile_passes;
    L->chunksP = sort_num_chunks(P);
    L->chunksI = sort_num_chunks(I);
    size_t o = 0;
    auto take = [&](size_t b) { size_t r = o; o += align_up(b); return r; };
    // geom
    L->g_keyA = take(4 * Pn);
    L->g_keyB = take(4 * Pn);
    L->g_valA = take(4 * Pn);
    L->g_valB = take(4 * Pn);
    L->pub.sorted_idx = L->g_valA;  // 4 passes: A -> B -> A -> B -> A
    L->pub.depth_key = L->g_keyA;   // (clobbered by the sort; kept for the layout struct only)
    L->pub.xy = take(16 * SPLAT_REC * Pn);      // one 64-byte record per Gaussian: xyh | conic+opacity | rgb+depth | pad
    L->pub.conic_opacity = L->pub.xy + 16;
    L->pub.rgbd = L->pub.xy + 32;
    L->pub.splat_stride = 16 * SPLAT_REC;
    L->pub.clamped = take(Pn);
    L->pub.tiles_touched = take(4 * Pn);
    L->pub.offsets = take(4 * Pn);
    L->g_hist = take(4 * (size_t)RADIX_SIZE * (size_t)(L->chunksP > 0 ? L->chunksP : 1));
    L->g_totals = take(4 * RADIX_SIZE);
    L->g_blocksums = take(4 * (size_t)div_up((int64_t)Pn, 4096));
    L->g_count = take(256);
    L->g_off_by_gid = take(4 * Pn);
    L->g_rect = take(4 * Pn);
    L->g_dhist = take(4 * 256);
    L->g_ghist = take(4 * 4 * RADIX_SIZE);
    L->g_ticket = take(256);
    L->g_status = take(onesweep_status_bytes((int64_t)Pn, 4));
    L->g_scan_status = take(scan_status_bytes((int)Pn));
    L->g_ctrl_bytes = o - L->g_ghist;
    if (shjac) L->g_shjac = take(4 * 9 * Pn);   // (last: every other offset is the same with and without it)
    L->pub.geom_bytes = o;
    // binning
    o = 0;
    L->b_keyA = take(4 * In);
    L->b_keyB = take(4 * In);
    L->b_valA = take(4 * In);
    L->b_valB = take(4 * In);
    L->b_hist = take(4 * (size_t)RADIX_SIZE * (size_t)(L->chunksI > 0 ? L->chunksI : 1));
    L->b_totals = take(4 * RADIX_SIZE);
    L->b_gid_of = take(4 * In);
    L->b_slot = take(4 * In);
    L->b_e2 = take(4 * In);
    L->b_ghist = take(4 * 4 * RADIX_SIZE);
    L->b_ticket = take(256);
    L->cursor_stride = I >= (int64_t)(1 << 20) ? CURSOR_STRIDE : 1;
    L->b_cursor = take(4 * (size_t)RADIX_SIZE * (size_t)L->cursor_stride);
    L->b_status = take(onesweep_status_bytes((int64_t)In, L->tile_passes + 1));   // (+ 1: the segmented path may take one more pass)
    L->b_ctrl_bytes = o - L->b_ghist;
    L->b_ckpt = take(((size_t)In / BUCKET + (size_t)(L->ntiles > 0 ? L->ntiles : 1) + 2) * 256 * 16);
    L->pub.binning_bytes = o;
    // ABI 16: behind it, what a forward with out_invdepth adds (Layout::d_*: the colour-only layout above is unchanged)
    const size_t npix_d = (size_t)W * (size_t)H;
    L->d_ckpt = take(((size_t)In / BUCKET + (size_t)(L->ntiles > 0 ? L->ntiles : 1) + 2) * 256 * 16);
    L->d_recs = take(16 * SPLAT_REC * Pn);
    L->d_dpix = take(4 * 3 * (npix_d > 0 ? npix_d : 1));
    L->d_bg = take(16);
    L->d_dz = take(4 * Pn);
    L->d_bytes = o;
    L->pub.point_list = (L->tile_passes & 1) ? L->b_valB : L->b_valA;
    // img
    o = 0;
    const size_t npix = (size_t)W * (size_t)H;
    L->pub.final_T = take(4 * (npix > 0 ? npix : 1));
    L->pub.n_contrib = take(4 * (npix > 0 ? npix : 1));
    L->pub.ranges = take(8 * (size_t)(L->ntiles > 0 ? L->ntiles : 1));
    L->i_order = take(4 * (size_t)(L->ntiles > 0 ? L->ntiles : 1));
    L->pub.img_bytes = o;
}

}  // namespace das3r

using namespace das3r;

extern "C" int das3r_abi_version(void) { return DAS3R_ABI_VERSION; }
extern "C" void das3r_reload_switches(void) { load_switches(); }
extern "C" void das3r_debug_inject_fault(uint32_t bits) {
    g_inject_fault = (int)bits;
    load_switches();
}
extern "C" void das3r_debug_mutate(uint32_t what) {
    g_mutate = (int)what;
    load_switches();
}
extern "C" const char *das3r_last_error(void) { return g_err; }
extern "C" int das3r_split_colour_switch(void) { return switches().split_colour; }
extern "C" int das3r_split_colour_rule(int32_t has_sh, int32_t sh_degree, int32_t P, int32_t binning_path, int32_t no_backward, int32_t forced) {
    return split_colour_rule(has_sh != 0, sh_degree, P, binning_path, no_backward != 0, forced) ? 1 : 0;
}

// The functions of path_policy.h on a caller's own state (include/das3r_raster.h): no HIP call, no look at this thread's PerDevice state or at
// the switches — everything the policy reads is in the two structs.
namespace {
struct PolicyOnState {
    Verdict v;
    Resume r;
    das3r_path_policy_state *s;
    explicit PolicyOnState(das3r_path_policy_state *state) : s(state) { policy_state_from(*s, &v, &r); }
    ~PolicyOnState() { policy_state_to(v, r, s); }
    PolicyInputs inputs(const das3r_path_policy_inputs *in) {
        return PolicyInputs{in->P, in->W, in->H, in->ntiles, in->tbits, in->tile_passes, in->too_long, in->want_bits, in->forced, in->onesweep != 0,
                            in->capacity_hint, in->capacity_exact != 0, &r};
    }
};
ForwardPlan plan_of(const das3r_path_policy_plan *p) {
    return ForwardPlan{p->local != 0, p->seg != 0, p->seg == 2, p->seg == 2 && p->cells != 0, p->seg_bits, p->seg_passes, p->speculate != 0, p->cap, p->decide_fine != 0, p->gen};
}
}  // namespace
extern "C" void das3r_debug_path_policy_fresh(das3r_path_policy_state *state, uint32_t gen) { policy_state_to(Verdict::fresh(gen), Resume(), state); }
extern "C" void das3r_debug_path_policy_plan(das3r_path_policy_state *state, const das3r_path_policy_inputs *in, das3r_path_policy_plan *out) {
    PolicyOnState on(state);
    const ForwardPlan p = plan_forward(on.v, on.inputs(in));
    *out = das3r_path_policy_plan{p.local, p.bucket_local ? 2 : (p.seg ? 1 : 0), p.seg_bits, p.seg_passes, p.speculate, p.decide_fine, p.gen, p.cells, p.cap};
}
extern "C" int das3r_debug_path_policy_count(das3r_path_policy_state *state, const das3r_path_policy_inputs *in, const das3r_path_policy_plan *plan, int64_t I) {
    PolicyOnState on(state);
    return learn_count(on.v, I, on.inputs(in), plan_of(plan)) ? 1 : 0;
}
extern "C" int das3r_debug_path_policy_skew(das3r_path_policy_state *state, uint32_t longest, uint32_t crowd16, int64_t cap, int32_t ntiles) {
    PolicyOnState on(state);
    return learn_skew(on.v, longest, crowd16, cap, ntiles) ? 1 : 0;
}
extern "C" uint32_t das3r_debug_path_policy_hint(const das3r_path_policy_state *state) {
    Verdict v;
    Resume r;
    policy_state_from(*state, &v, &r);
    return backward_hint(v, (uint32_t)BUCKET);
}
extern "C" void das3r_debug_path_policy_forget(das3r_path_policy_state *state) {
    PolicyOnState on(state);
    forget(on.v);
}
extern "C" void das3r_debug_path_policy_resume(das3r_path_policy_state *state, uint32_t fine, uint32_t forwards) {
    PolicyOnState on(state);
    resume(on.v, on.r, fine != 0u, forwards);
}
extern "C" int das3r_debug_seg_dbits(int32_t tbits, int32_t passes) { return seg_dbits((int)tbits, (int)passes); }

// The functions of kernel_choice.h on a caller's own switches (include/das3r_raster.h): no HIP call, no look at the process environment or at
// the switches the library itself last read.
extern "C" void das3r_debug_parse_switches(const char *const *names, const char *const *values, int32_t n, int32_t experiments, das3r_switches *out) {
    auto lookup = [&](const char *name) -> const char * {
        for (int32_t i = 0; i < n; i++)
            if (strcmp(names[i], name) == 0) return values[i];
        return nullptr;
    };
    switches_to(parse_switches(lookup, experiments != 0), out);
}
extern "C" void das3r_debug_choose_backward(const das3r_switches *sw, int64_t num_rendered, int32_t ntiles, uint32_t fwd_flags, das3r_bwd_choice *out) {
    const BwdChoice c = choose_backward(switches_from(*sw), num_rendered, ntiles, fwd_flags);
    *out = das3r_bwd_choice{c.kernel, c.mb, c.slices, c.pix, c.occ, c.strips, c.atomic_flush};
}
extern "C" void das3r_debug_choose_forward(const das3r_switches *sw, int32_t ntiles, int64_t capacity, int32_t local_lists, int32_t prefer_regions,
                                           das3r_fwd_choice *out) {
    const Switches w = switches_from(*sw);
    const bool local = local_lists != 0, regions = prefer_regions != 0;
    *out = das3r_fwd_choice{choose_forward(w, ntiles, capacity, local, regions), quad_lanes(w, ntiles, capacity, local), row_private(w, capacity, ntiles),
                            tile_lpt_wanted(w, ntiles, capacity, local, regions)};
}
extern "C" int das3r_debug_has_invdepth_form(int32_t backward, int32_t kernel) {
    return (backward ? bwd_has_invdepth_form((BwdKernel)kernel) : fwd_has_invdepth_form((FwdKernel)kernel)) ? 1 : 0;
}
extern "C" const char *das3r_debug_kernel_name(int32_t backward, int32_t kernel) {
    return backward ? bwd_kernel_name((BwdKernel)kernel) : fwd_kernel_name((FwdKernel)kernel);
}

// The functions of preprocess_choice.h on a caller's own values: which form of preprocess_backward_kernel a backward launches, and its raw name
static PreprocessForm form_from(const das3r_preprocess_form *f) {
    return PreprocessForm{f->has_sh != 0, f->has_cov != 0, f->stage_in != 0, f->stage_out != 0, f->deg0 != 0, f->chain != 0, f->depth != 0, f->jac != 0, f->aa != 0};
}
extern "C" int das3r_debug_choose_preprocess_backward(const das3r_preprocess_backward_inputs *in, das3r_preprocess_form *out) {
    const PreprocessBackwardInputs ci = {in->has_sh != 0, in->has_cov != 0, in->M, in->sh_degree, in->shs_aligned16 != 0, in->dL_dshs_aligned16 != 0,
                                         in->no_sh_stage != 0, in->jac_saved != 0, in->chained != 0, in->quad_rows != 0, in->depth != 0, in->aa != 0};
    const PreprocessForm f = choose_preprocess_backward(ci);
    *out = das3r_preprocess_form{f.has_sh, f.has_cov, f.stage_in, f.stage_out, f.deg0, f.chain, f.depth, f.jac, f.aa, preprocess_backward_base_index(f),
                                 sh_rows_staged(ci.has_sh, ci.M, ci.sh_degree, ci.shs_aligned16, ci.no_sh_stage)};
    return chain_refusal(ci);
}
extern "C" const char *das3r_debug_preprocess_backward_name(const das3r_preprocess_form *form) { return preprocess_backward_name(form_from(form)); }

extern "C" int das3r_raster_get_layout(int32_t P, int64_t num_rendered, int32_t W, int32_t H, das3r_raster_layout *out) {
    if (!out || P < 0 || num_rendered < 0 || W <= 0 || H <= 0) { set_error("das3r_raster_get_layout: invalid argument"); return DAS3R_ERR_INVALID_ARG; }
    Layout L;
    compute_layout(P, num_rendered, W, H, &L);
    *out = L.pub;
    return DAS3R_OK;
}

// ABI 13: what the calling thread's library state has LEARNT about shapes on the current device is forgotten (counts, binning path, forward
// kernel choice); the mailbox, rings and tickets stay.  See include/das3r_raster.h.
extern "C" int das3r_raster_forget_shapes(void) {
    PerDevice *T = nullptr;
    int r = per_device(&T);
    if (r) return r;
    forget(T->verdict);
    return DAS3R_OK;
}

// ABI 13: the part of the learnt state that shows in the last bit of a result — the forward kernel of the current shape and the position in its
// re-decision schedule.  set == 0: read into state[0 .. 1]; set != 0: forget the shapes and hand state[] to the next shape this thread meets.
extern "C" int das3r_raster_learning(int32_t set, uint32_t state[2]) {
    if (!state) { set_error("das3r_raster_learning: invalid argument"); return DAS3R_ERR_INVALID_ARG; }
    PerDevice *T = nullptr;
    int r = per_device(&T);
    if (r) return r;
    if (!set) {
        state[0] = prefers_regions(T->verdict) ? 1u : 0u;
        state[1] = forwards_seen(T->verdict);
        return DAS3R_OK;
    }
    resume(T->verdict, T->resume, state[0] != 0u, state[1]);
    return DAS3R_OK;
}

// The view of a finished forward's buffers: laid out for the capacity they were laid out for (a caller that kept only num_rendered: for that).
// (rasterizer.py alpha_of asks das3r_raster_get_layout the same way.)  in (may be null: an entry that never reads the Jacobian planes) — flags
// bit 2: the forward left the SH colour's Jacobian for the per-Gaussian backward (Layout::g_shjac), which then reads it instead of the SH rows.
// Without it (a caller that handed back flags = 0) the backward reads the rows as before.
static Buffers saved_buffers(const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_saved *saved) {
    const bool shjac = in && (saved->flags & SHJAC_SAVED_FLAG) != 0 && in->shs != nullptr && a->sh_degree >= 2;
    Buffers v = {saved->geom, saved->binning, saved->img, saved->geom, {}};
    compute_layout(a->P, saved->capacity > 0 ? saved->capacity : saved->num_rendered, a->image_width, a->image_height, &v.L, shjac);
    return v;
}

// What das3r_raster_backward (depth_pass false; dL_dinvdepth not looked at) and das3r_raster_backward_depth ask of their pointers.
static int backward_validate(const char *who, const das3r_raster_in *in, const das3r_raster_saved *saved, const float *dL_dpix, bool depth_pass,
                             const float *dL_dinvdepth, const das3r_raster_grads *g) {
    const bool chained = g && g->chain;   // (ABI 14: dL/d(camera-frame means, opacities, scales, rotations) are then not produced — may be NULL)
    if (!saved || !saved->geom || !saved->img || !dL_dpix || (depth_pass && !dL_dinvdepth) || !g || !g->dL_dmeans2D ||
        (!chained && (!g->dL_dopacities || !g->dL_dmeans3D)) || (saved->num_rendered > 0 && !g->scratch)) {
        set_error("%s: null saved state / %sgradient buffer", who, depth_pass ? "upstream gradient / " : "");
        return DAS3R_ERR_INVALID_ARG;
    }
    if (depth_pass && !(saved->flags & DEPTH_SAVED_FLAG)) {
        set_error("%s: the saved state is not that of a forward with out_invdepth (das3r_raster_saved.flags bit 1 is clear)", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    const bool has_sh = in->shs != nullptr, has_cov = in->cov3D_precomp != nullptr;
    if ((has_sh && !g->dL_dshs) || (!has_sh && !g->dL_dcolors_precomp) || (has_cov && !g->dL_dcov3D) ||
        (!has_cov && !chained && (!g->dL_dscales || !g->dL_drotations))) {
        set_error("%s: gradient buffer missing for a provided input", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    return DAS3R_OK;
}

// What das3r_raster_backward_focal adds to a backward (focal_grad.hip); null for the two entries that do not.
struct FocalOut {
    float *sums, *per_splat, *workspace;
};

// the depth pass runs the compositing backward a second time: a forced kernel must have an inverse-depth form (kernel_choice.h)
static int refuse_bwd_without_invdepth(const char *who) {
    const BwdKernel k = switches().render_bwd;
    if (bwd_has_invdepth_form(k)) return DAS3R_OK;
    set_error("%s: DAS3R_RENDER_BWD=%s has no inverse-depth form", who, bwd_kernel_name(k));
    return DAS3R_ERR_INVALID_ARG;
}

// The nine-float rows of partial sums, one per instance, + 16 bytes (the per-Gaussian backward reads the rows of a workgroup as 16-byte words up
// to the boundary above the last row); rows_aligned: the same rounded up — where whatever a call keeps behind the rows starts.
static size_t rows_bytes(int64_t capacity) { return (capacity > 0 ? (size_t)capacity : 1) * 9 * sizeof(float) + 16; }
static size_t rows_aligned(int64_t capacity) { return align_up(rows_bytes(capacity)); }
static float *behind_rows(float *scratch, const Buffers &v) { return (float *)((char *)scratch + rows_aligned(v.L.capacity)); }

// What the backward entries that end in launch_preprocess_backward do first: the refusals in their order, then the view of the saved buffers.
// P == 0: DAS3R_OK at once, *v untouched.  binning_first: a missing binning buffer is refused before the binning self-check, not after it.
static int backward_prologue(const char *who, const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_saved *saved, const float *dL_dpix,
                             bool depth_pass, const float *dL_dinvdepth, const das3r_raster_grads *g, bool binning_first, das3r_stream_t stream, Buffers *v) {
    int rc = validate(a, in);
    if (rc || a->P == 0) return rc;
    if ((rc = backward_validate(who, in, saved, dL_dpix, depth_pass, dL_dinvdepth, g))) return rc;
    if (depth_pass && (rc = refuse_bwd_without_invdepth(who))) return rc;
    const bool no_binning = saved->num_rendered > 0 && !saved->binning;
    // the forward's binning self-check first: nothing is launched on the strength of an invalid image / list
    if (!(no_binning && binning_first) && (rc = das3r_raster_check(saved, stream))) return rc;
    if (no_binning) { set_error("%s: binning buffer missing", who); return DAS3R_ERR_INVALID_ARG; }
    *v = saved_buffers(a, in, saved);
    return DAS3R_OK;
}

// The backward pass of das3r_raster_backward (depth_pass false), das3r_raster_backward_depth (true) and das3r_raster_backward_focal (either,
// with `focal`): the launches of the first two are what they were, the third puts one per-Gaussian kernel and its finish between the
// compositing passes (+ the depth fold) and the per-Gaussian backward — before grads->chain's Adam step touches the parameters it reads.
//
// ABI 16, the depth pass: the backward of (colour, inverse depth).  The colour pass is das3r_raster_backward's; the depth pass is the same compositing backward
// (the same kernel: the choice depends on the lists and the flags only) on the colour (1/z, 0, 0) with background 0, upstream gradient
// (dL/dinvdepth, 0, 0) and the depth checkpoints — preprocess_bwd.hip depth_pass_inputs_kernel / depth_fold_kernel say why that is the
// backward of the fourth channel.  Its geometry sums are added to the colour pass's rows, its colour sums become dL/dz, which the per-Gaussian
// kernel adds to dL/dmeans3D (before the chain, with grads->chain).  Everything it writes besides grads and scratch is in the binning
// buffer's depth part (Layout::d_*), which only a forward with out_invdepth has: das3r_raster_saved.flags bit 1 says so.
static int backward_body(const char *who, const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_saved *saved, const float *dL_dpix,
                         bool depth_pass, const float *dL_dinvdepth, const das3r_raster_grads *g, const FocalOut *focal, das3r_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    Buffers v;
    int rc = backward_prologue(who, a, in, saved, dL_dpix, depth_pass, dL_dinvdepth, g, false, stream, &v);
    if (rc) return rc;
    const int P = a->P;
    if (P == 0) {
        if (focal) HIP_TRY(hipMemsetAsync(focal->sums, 0, 2 * sizeof(float), s));   // (per_splat has no element)
        return DAS3R_OK;
    }
    // scratch = per-instance partial sums [num_rendered, 9]; no accumulator needs zeroing (no atomics anywhere)
    float *partial = g->scratch;
    const float *dz = nullptr;
    bool quad_rows = false;
    if (saved->num_rendered > 0) {
        if ((rc = launch_render_backward(a, dL_dpix, v, partial, s, &quad_rows, saved->num_rendered, saved->flags))) return rc;
        if (depth_pass) {
            float *partial_depth = behind_rows(g->scratch, v);
            if ((rc = launch_depth_pass_inputs(P, a->image_width * a->image_height, v, dL_dinvdepth, s, a->debug != 0))) return rc;
            das3r_raster_args ad = *a;
            const Buffers vd = v.depth_pass(&ad);   // its splat records, checkpoints and background (ad.bg): the binning buffer's depth part
            bool quad_rows_d = false;
            if ((rc = launch_render_backward(&ad, v.d_dpix(), vd, partial_depth, s, &quad_rows_d, saved->num_rendered, saved->flags))) return rc;
            float *dzw = v.d_dz();
            if ((rc = launch_depth_fold(P, v, partial, partial_depth, dzw, s, a->debug != 0))) return rc;
            dz = dzw;
        }
    }
    const bool aa = (saved->flags & ANTIALIAS_FLAG) != 0;
    // (nothing rendered: tiles_touched is all zero, the kernel reads no row and writes the zeros)
    if (focal && (rc = launch_focal_grad(a, in, v, partial, quad_rows, aa, focal->sums, focal->per_splat, focal->workspace, s))) return rc;
    // (the depth pass's opacity sums were folded into `partial` above: the antialiasing factor's derivative is applied once, to the total)
    return launch_preprocess_backward(a, in, v, g, partial, s, quad_rows, dz, aa);
}

extern "C" int das3r_raster_backward(const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_saved *saved,
                                     const float *dL_dpix, const das3r_raster_grads *g, das3r_stream_t stream) {
    return backward_body("das3r_raster_backward", a, in, saved, dL_dpix, false, nullptr, g, nullptr, stream);
}

extern "C" int das3r_raster_backward_depth(const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_saved *saved,
                                           const float *dL_dpix, const float *dL_dinvdepth, const das3r_raster_grads *g, das3r_stream_t stream) {
    return backward_body("das3r_raster_backward_depth", a, in, saved, dL_dpix, true, dL_dinvdepth, g, nullptr, stream);
}

// Additive under ABI 16: the whole backward (das3r_raster_backward, or with dL_dinvdepth das3r_raster_backward_depth — the same launches, the
// same gradients bit for bit) plus dL/d(log-focal offsets) of the same loss: focal_grad.hip.  Refused before anything is launched: NULL sums /
// workspace, and with dL_dinvdepth the forced DAS3R_RENDER_BWD forms das3r_raster_backward_depth refuses.
extern "C" size_t das3r_raster_focal_workspace_bytes(int32_t P) { return focal_workspace_bytes(P); }
extern "C" int das3r_raster_backward_focal(const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_saved *saved, const float *dL_dpix,
                                           const float *dL_dinvdepth, const das3r_raster_grads *g, float *sums, float *per_splat, float *workspace,
                                           das3r_stream_t stream) {
    if (!sums || !workspace) {
        set_error("das3r_raster_backward_focal: null sums / workspace");
        return DAS3R_ERR_INVALID_ARG;
    }
    const bool depth_pass = dL_dinvdepth != nullptr;
    if (depth_pass) {   // (before the saved state is looked at, under this entry's own name)
        const int rc = refuse_bwd_without_invdepth("das3r_raster_backward_focal");
        if (rc) return rc;
    }
    const FocalOut focal = {sums, per_splat, workspace};
    return backward_body("das3r_raster_backward_focal", a, in, saved, dL_dpix, depth_pass, dL_dinvdepth, g, &focal, stream);
}

// das3r_raster_backward_scratch_bytes' rows twice: the colour pass's and the depth pass's (whose first column is the per-instance depth sum)
extern "C" size_t das3r_raster_backward_depth_scratch_bytes(int64_t capacity) {
    return rows_aligned(capacity) + rows_bytes(capacity);
}

// rows_bytes.  (The experimental stream kernel — EXPERIMENTS=1 builds, DAS3R_RENDER_BWD=stream — needs up to four 48-byte rows per
// instance: only then is the larger figure returned.)
extern "C" size_t das3r_raster_backward_scratch_bytes(int64_t capacity) {
#ifdef DAS3R_EXPERIMENTS
    if (switches().render_bwd == BWD_STREAM) return std::max(rows_bytes(capacity), stream_scratch_bytes(capacity));
#endif
    return rows_bytes(capacity);
}

// ---- extra per-Gaussian channels over a forward's saved lists (render_aux.hip) ----
// Both calls read the saved state only (ranges, lists, n_contrib, splat records, emission slots, tiles_touched / off_by_gid): any number of
// them, before or after das3r_raster_backward / _depth, which read the same buffers and write none of what is read here.
static int aux_validate(const char *who, const das3r_raster_args *a, const das3r_raster_saved *saved, int32_t C, const void *p0, const void *p1) {
    if (!a || !saved) { set_error("%s: null args / saved state", who); return DAS3R_ERR_INVALID_ARG; }
    if (C < 1 || C > DAS3R_AUX_MAX_CHANNELS) { set_error("%s: C = %d channels (1 .. %d per call)", who, C, DAS3R_AUX_MAX_CHANNELS); return DAS3R_ERR_INVALID_ARG; }
    if (a->P < 0 || a->image_width <= 0 || a->image_height <= 0) { set_error("%s: bad extents P=%d W=%d H=%d", who, a->P, a->image_width, a->image_height); return DAS3R_ERR_INVALID_ARG; }
    if (!p1 || (a->P > 0 && !p0)) { set_error("%s: null feature / image / gradient pointer", who); return DAS3R_ERR_INVALID_ARG; }
    if (a->P > 0 && saved->num_rendered > 0 && (!saved->geom || !saved->binning || !saved->img)) { set_error("%s: saved buffers missing", who); return DAS3R_ERR_INVALID_ARG; }
    return DAS3R_OK;
}

extern "C" int das3r_raster_aux_forward(const das3r_raster_args *a, const das3r_raster_saved *saved, int32_t C, const float *features, float *out,
                                        das3r_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = aux_validate("das3r_raster_aux_forward", a, saved, C, features, out);
    if (rc) return rc;
    const int P = a->P, W = a->image_width, H = a->image_height;
    if (P == 0 || saved->num_rendered <= 0) {   // nothing was blended: an empty image (upstream's empty scene)
        HIP_TRY(hipMemsetAsync(out, 0, sizeof(float) * (size_t)C * (size_t)W * (size_t)H, s));
        return DAS3R_OK;
    }
    if ((rc = das3r_raster_check(saved, stream))) return rc;   // a failed binning is an error, not a walk over bad lists
    const Buffers v = saved_buffers(a, nullptr, saved);
    return launch_render_aux_forward(P, W, H, C, features, out, v, saved->num_rendered, a->debug != 0, s);
}

// C floats per instance + 16 bytes (as das3r_raster_backward_scratch_bytes rounds its rows up)
extern "C" size_t das3r_raster_aux_scratch_bytes(int64_t capacity, int32_t C) {
    const size_t c = capacity > 0 ? (size_t)capacity : 1, ch = C > 0 ? (size_t)C : 1;
    return c * ch * sizeof(float) + 16;
}

extern "C" int das3r_raster_aux_adjoint(const das3r_raster_args *a, const das3r_raster_saved *saved, int32_t C, const float *dL_dout, float *dL_dfeat,
                                        int32_t accumulate, float *scratch, das3r_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = aux_validate("das3r_raster_aux_adjoint", a, saved, C, dL_dfeat, dL_dout);
    if (rc) return rc;
    const int P = a->P, W = a->image_width, H = a->image_height;
    if (P == 0) return DAS3R_OK;   // dL_dfeat has no rows
    if (saved->num_rendered <= 0) {
        if (!accumulate) HIP_TRY(hipMemsetAsync(dL_dfeat, 0, sizeof(float) * (size_t)P * (size_t)C, s));
        return DAS3R_OK;
    }
    if (!scratch) { set_error("das3r_raster_aux_adjoint: null scratch (das3r_raster_aux_scratch_bytes)"); return DAS3R_ERR_INVALID_ARG; }
    if ((rc = das3r_raster_check(saved, stream))) return rc;
    const Buffers v = saved_buffers(a, nullptr, saved);
    return launch_render_aux_adjoint(P, W, H, C, dL_dout, dL_dfeat, accumulate != 0, scratch, v, saved->num_rendered, a->debug != 0, s);
}

// ---- the aux channels' and the coverage image's gradients to the geometry (render_aux_bwd.hip) ----
// Additive under ABI 16.  The whole backward of L = <dL_dout, aux image> + <dL_dalpha, 1 - final_T> for the forward that left `saved`: one
// compositing kernel (rows 3..8 of the nine-float rows, 0..2 zero; with dL_dfeatures the [capacity, C] feature rows on the same walk), the
// gather for dL_dfeatures, then the per-Gaussian backward exactly as a colour loss runs it (quad_rows false, no depth term, the forward's
// antialiasing flag).  Scratch: the nine-float rows as das3r_raster_backward_scratch_bytes rounds them, then the feature rows.
extern "C" size_t das3r_raster_aux_backward_scratch_bytes(int64_t capacity, int32_t C) {
    const size_t c = capacity > 0 ? (size_t)capacity : 1, ch = C > 0 ? (size_t)C : 0;
    return rows_aligned(capacity) + c * ch * sizeof(float) + 16;
}

extern "C" int das3r_raster_aux_backward(const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_saved *saved, int32_t C,
                                         const float *features, const float *dL_dout, const float *dL_dalpha, float *dL_dfeatures,
                                         const das3r_raster_grads *g, das3r_stream_t stream) {
    static const char who[] = "das3r_raster_aux_backward";
    hipStream_t s = (hipStream_t)stream;
    if (!a || !in || !saved || !g) { set_error("%s: null args / inputs / saved state / grads", who); return DAS3R_ERR_INVALID_ARG; }
    if (C < 0 || C > DAS3R_AUX_MAX_CHANNELS) { set_error("%s: C = %d channels (0 .. %d per call)", who, C, DAS3R_AUX_MAX_CHANNELS); return DAS3R_ERR_INVALID_ARG; }
    if (C == 0 && !dL_dalpha) { set_error("%s: C = 0 channels and null dL_dalpha: no loss term", who); return DAS3R_ERR_INVALID_ARG; }
    if (C == 0 && dL_dfeatures) { set_error("%s: dL_dfeatures with C = 0 channels", who); return DAS3R_ERR_INVALID_ARG; }
    if (C > 0 && (!dL_dout || (a->P > 0 && !features))) { set_error("%s: null features / dL_dout with C = %d channels", who, C); return DAS3R_ERR_INVALID_ARG; }
    if (g->chain) { set_error("%s: grads->chain is not supported here (the chained backward belongs to the colour loss)", who); return DAS3R_ERR_INVALID_ARG; }
    if (!g->scratch) { set_error("%s: null scratch (das3r_raster_aux_backward_scratch_bytes)", who); return DAS3R_ERR_INVALID_ARG; }
    Buffers v;
    int rc = backward_prologue(who, a, in, saved, /*dL_dpix: not this entry's*/ g->scratch, false, nullptr, g, true, stream, &v);
    const int P = a->P, W = a->image_width, H = a->image_height;
    if (rc || P == 0) return rc;   // (P == 0: no gradient has a row)
    float *partial = g->scratch;
    if (saved->num_rendered > 0) {
        float *partial_f = dL_dfeatures ? behind_rows(g->scratch, v) : nullptr;
        if ((rc = launch_render_aux_backward(P, W, H, C, features, dL_dout, dL_dalpha, partial, partial_f, v, a->debug != 0, s))) return rc;
        if (dL_dfeatures && (rc = launch_aux_gather(P, C, partial_f, dL_dfeatures, v, a->debug != 0, s))) return rc;
    } else if (dL_dfeatures) {
        HIP_TRY(hipMemsetAsync(dL_dfeatures, 0, sizeof(float) * (size_t)P * (size_t)C, s));
    }
    // (nothing rendered: tiles_touched is all zero, the kernel reads no row and writes the zeros; columns 0..2 are zero: so is dL/d(colour, SH))
    return launch_preprocess_backward(a, in, v, g, partial, s, false, nullptr, (saved->flags & ANTIALIAS_FLAG) != 0);
}

// ---- the ray-distortion regulariser over a forward's saved lists (render_distort.hip) ----
// Additive under ABI 16; include/das3r_raster.h fixes the definition.  The forward call reads the saved state only, as das3r_raster_aux_forward
// does; the backward call is das3r_raster_aux_backward's sequence with one more step: the compositing kernel leaves the per-instance dL/dm sums
// in column 0 of the nine-float rows, the fold turns them into dz [P] behind the rows — caller scratch, not the binning buffer's depth part,
// which a colour-only forward does not have — and the per-Gaussian backward takes dz as the depth pass's.
extern "C" int das3r_raster_distortion_forward(const das3r_raster_args *a, const das3r_raster_saved *saved, float *out, float *totals,
                                               das3r_stream_t stream) {
    static const char who[] = "das3r_raster_distortion_forward";
    hipStream_t s = (hipStream_t)stream;
    if (!a || !saved) { set_error("%s: null args / saved state", who); return DAS3R_ERR_INVALID_ARG; }
    if (a->P < 0 || a->image_width <= 0 || a->image_height <= 0) { set_error("%s: bad extents P=%d W=%d H=%d", who, a->P, a->image_width, a->image_height); return DAS3R_ERR_INVALID_ARG; }
    if (!out) { set_error("%s: null image pointer", who); return DAS3R_ERR_INVALID_ARG; }
    if (a->P > 0 && saved->num_rendered > 0 && (!saved->geom || !saved->binning || !saved->img)) { set_error("%s: saved buffers missing", who); return DAS3R_ERR_INVALID_ARG; }
    const int P = a->P, W = a->image_width, H = a->image_height;
    if (P == 0 || saved->num_rendered <= 0) {   // nothing was blended: no pair anywhere
        HIP_TRY(hipMemsetAsync(out, 0, sizeof(float) * (size_t)W * (size_t)H, s));
        if (totals) HIP_TRY(hipMemsetAsync(totals, 0, sizeof(float) * (size_t)W * (size_t)H, s));
        return DAS3R_OK;
    }
    int rc = das3r_raster_check(saved, stream);   // a failed binning is an error, not a walk over bad lists
    if (rc) return rc;
    const Buffers v = saved_buffers(a, nullptr, saved);
    return launch_render_distortion_forward(P, W, H, out, totals, v, a->debug != 0, s);
}

// the nine-float rows as das3r_raster_backward_scratch_bytes rounds them, then dz: one float per Gaussian
extern "C" size_t das3r_raster_distortion_backward_scratch_bytes(int64_t capacity, int32_t P) {
    return rows_aligned(capacity) + (P > 0 ? (size_t)P : 0) * sizeof(float) + 16;
}

extern "C" int das3r_raster_distortion_backward(const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_saved *saved,
                                                const float *dL_ddist, const float *totals, const das3r_raster_grads *g, das3r_stream_t stream) {
    static const char who[] = "das3r_raster_distortion_backward";
    hipStream_t s = (hipStream_t)stream;
    if (!a || !in || !saved || !g) { set_error("%s: null args / inputs / saved state / grads", who); return DAS3R_ERR_INVALID_ARG; }
    if (!dL_ddist || !totals) { set_error("%s: null dL_ddist / totals plane (das3r_raster_distortion_forward writes it)", who); return DAS3R_ERR_INVALID_ARG; }
    if (g->chain) { set_error("%s: grads->chain is not supported here (the chained backward belongs to the colour loss)", who); return DAS3R_ERR_INVALID_ARG; }
    if (!g->scratch) { set_error("%s: null scratch (das3r_raster_distortion_backward_scratch_bytes)", who); return DAS3R_ERR_INVALID_ARG; }
    Buffers v;
    int rc = backward_prologue(who, a, in, saved, /*dL_dpix: not this entry's*/ dL_ddist, false, nullptr, g, true, stream, &v);
    const int P = a->P, W = a->image_width, H = a->image_height;
    if (rc || P == 0) return rc;   // (P == 0: no gradient has a row)
    float *partial = g->scratch;
    const float *dz = nullptr;
    if (saved->num_rendered > 0) {
        float *dzw = behind_rows(g->scratch, v);
        if ((rc = launch_render_distortion_backward(P, W, H, dL_ddist, totals, partial, v, a->debug != 0, s))) return rc;
        if ((rc = launch_distortion_fold(P, v, partial, dzw, a->debug != 0, s))) return rc;
        dz = dzw;
    }
    // (nothing rendered: tiles_touched is all zero, the kernel reads no row and writes the zeros; columns 0..2 are zero: so is dL/d(colour, SH))
    return launch_preprocess_backward(a, in, v, g, partial, s, false, dz, (saved->flags & ANTIALIAS_FLAG) != 0);
}

// ---- median depth and surface hits over a forward's saved lists (render_median.hip) ----
// Additive under ABI 16; include/das3r_raster.h fixes the definition.  Both calls read the saved state only, as das3r_raster_aux_forward /
// das3r_raster_aux_adjoint do; the adjoint is the aux adjoint's sequence: one compositing kernel into per-instance rows, then the gather.
static int median_validate(const char *who, const das3r_raster_args *a, const das3r_raster_saved *saved) {
    if (!a || !saved) { set_error("%s: null args / saved state", who); return DAS3R_ERR_INVALID_ARG; }
    if (a->P < 0 || a->image_width <= 0 || a->image_height <= 0) { set_error("%s: bad extents P=%d W=%d H=%d", who, a->P, a->image_width, a->image_height); return DAS3R_ERR_INVALID_ARG; }
    return DAS3R_OK;
}
static int median_buffers(const char *who, const das3r_raster_args *a, const das3r_raster_saved *saved) {
    if (a->P > 0 && saved->num_rendered > 0 && (!saved->geom || !saved->binning || !saved->img)) { set_error("%s: saved buffers missing", who); return DAS3R_ERR_INVALID_ARG; }
    return DAS3R_OK;
}

extern "C" int das3r_raster_median_forward(const das3r_raster_args *a, const das3r_raster_saved *saved, float threshold, float *depth,
                                           int32_t *hit_gaussian, uint32_t *hit_position, das3r_stream_t stream) {
    static const char who[] = "das3r_raster_median_forward";
    hipStream_t s = (hipStream_t)stream;
    int rc = median_validate(who, a, saved);
    if (rc) return rc;
    if (!depth) { set_error("%s: null depth pointer", who); return DAS3R_ERR_INVALID_ARG; }
    if (!(threshold > 0.0f && threshold < 1.0f)) { set_error("%s: threshold %g is not inside (0, 1)", who, (double)threshold); return DAS3R_ERR_INVALID_ARG; }
    if ((rc = median_buffers(who, a, saved))) return rc;
    const int P = a->P, W = a->image_width, H = a->image_height;
    if (P == 0 || saved->num_rendered <= 0) {   // nothing was blended: every pixel is empty (0 / -1 / 0xFFFFFFFF)
        const size_t npix = (size_t)W * (size_t)H;
        HIP_TRY(hipMemsetAsync(depth, 0, sizeof(float) * npix, s));
        if (hit_gaussian) HIP_TRY(hipMemsetAsync(hit_gaussian, 0xFF, sizeof(int32_t) * npix, s));
        if (hit_position) HIP_TRY(hipMemsetAsync(hit_position, 0xFF, sizeof(uint32_t) * npix, s));
        return DAS3R_OK;
    }
    if ((rc = das3r_raster_check(saved, stream))) return rc;   // a failed binning is an error, not a walk over bad lists
    const Buffers v = saved_buffers(a, nullptr, saved);
    return launch_render_median_forward(P, W, H, threshold, depth, hit_gaussian, hit_position, v, a->debug != 0, s);
}

// one float per instance + 16 bytes (as das3r_raster_aux_scratch_bytes rounds its rows up)
extern "C" size_t das3r_raster_median_scratch_bytes(int64_t capacity) {
    return (capacity > 0 ? (size_t)capacity : 1) * sizeof(float) + 16;
}

extern "C" int das3r_raster_median_adjoint(const das3r_raster_args *a, const das3r_raster_saved *saved, const float *dL_ddepth,
                                           const uint32_t *hit_position, float *dL_dz, int32_t accumulate, float *scratch, das3r_stream_t stream) {
    static const char who[] = "das3r_raster_median_adjoint";
    hipStream_t s = (hipStream_t)stream;
    int rc = median_validate(who, a, saved);
    if (rc) return rc;
    if (!dL_ddepth || !hit_position) { set_error("%s: null dL_ddepth / hit_position plane (das3r_raster_median_forward writes it)", who); return DAS3R_ERR_INVALID_ARG; }
    if (a->P > 0 && !dL_dz) { set_error("%s: null dL_dz pointer", who); return DAS3R_ERR_INVALID_ARG; }
    if (!scratch) { set_error("%s: null scratch (das3r_raster_median_scratch_bytes)", who); return DAS3R_ERR_INVALID_ARG; }
    if ((rc = median_buffers(who, a, saved))) return rc;
    const int P = a->P, W = a->image_width, H = a->image_height;
    if (P == 0) return DAS3R_OK;   // dL_dz has no rows
    if (saved->num_rendered <= 0) {
        if (!accumulate) HIP_TRY(hipMemsetAsync(dL_dz, 0, sizeof(float) * (size_t)P, s));
        return DAS3R_OK;
    }
    if ((rc = das3r_raster_check(saved, stream))) return rc;
    const Buffers v = saved_buffers(a, nullptr, saved);
    return launch_render_median_adjoint(P, W, H, dL_ddepth, hit_position, dL_dz, accumulate != 0, scratch, v, a->debug != 0, s);
}

extern "C" int das3r_has_experiments(void) {
#ifdef DAS3R_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

extern "C" int das3r_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                                  uint8_t *present, das3r_stream_t stream) {
    (void)projmatrix;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) { set_error("das3r_mark_visible: invalid argument"); return DAS3R_ERR_INVALID_ARG; }
    return launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
}

// ---- test aid: fill every CU's LDS with a bit pattern ----
// The compositing kernels leave parts of their LDS arrays unwritten (list tails, staged entries past a tile's list); what they
// then read must not matter.  A test fills the LDS of every CU with NaNs / all-ones first (tests/test_gpu_raster.py).
__global__ void __launch_bounds__(1024) poison_lds_kernel(uint32_t pattern, uint32_t *sink, int words) {
    extern __shared__ uint32_t lds_words[];
    for (int i = threadIdx.x; i < words; i += 1024) lds_words[i] = pattern;
    __syncthreads();
    if (lds_words[(threadIdx.x * 37) % words] != pattern) *sink = 1u;       // (keeps the stores alive)
}
extern "C" int das3r_debug_poison_lds(uint32_t pattern, das3r_stream_t stream) {
    // per device: the sink lives on the device the call runs on, and the fill is as large as that device lets one workgroup have
    static uint32_t *sinks[MAX_DEVICES] = {};
    int dev = 0, lds_bytes = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) { set_error("device ordinal %d not supported", dev); return DAS3R_ERR_INVALID_ARG; }
    HIP_TRY(hipDeviceGetAttribute(&lds_bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    const int words = lds_bytes / 4 - 64;   // just under the limit (160 KB per CU on MI355X)
    if (words <= 0) { set_error("das3r_debug_poison_lds: no LDS"); return DAS3R_ERR_HIP; }
    if (!sinks[dev]) HIP_TRY(hipMalloc((void **)&sinks[dev], 4));
    HIP_TRY(hipFuncSetAttribute((const void *)poison_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, words * 4));
    hipLaunchKernelGGL(poison_lds_kernel, dim3(1024), dim3(1024), words * 4, (hipStream_t)stream, pattern, sinks[dev], words);
    HIP_TRY(hipGetLastError());
    return DAS3R_OK;
}

// ---- pair counters ----
static unsigned long long *g_pairs = nullptr;
static int g_pairs_dev = -1;   // the counters live on ONE device (bench.py counts on its own GPU); launches on any other get none
namespace das3r {
unsigned long long *pair_counters() {
    if (!g_pairs) return nullptr;
    int dev = -1;
    return (hipGetDevice(&dev) == hipSuccess && dev == g_pairs_dev) ? g_pairs : nullptr;
}
}  // namespace das3r
// enable != 0: (allocate and) zero the counters, the compositing kernels count from now on; enable == 0: read them into out[4] (may be
// null), stop counting.  Single-threaded use (bench.py); synchronises the device.
extern "C" int das3r_pair_counters(int enable, uint64_t out[4]) {
    if (enable) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        if (g_pairs && dev != g_pairs_dev) { set_error("das3r_pair_counters: already counting on device %d", g_pairs_dev); return DAS3R_ERR_INVALID_ARG; }
        if (!g_pairs) HIP_TRY(hipMalloc((void **)&g_pairs, (4 + PHASE_WORDS * PHASE_COPIES) * sizeof(unsigned long long)));
        g_pairs_dev = dev;
        HIP_TRY(hipMemset(g_pairs, 0, (4 + PHASE_WORDS * PHASE_COPIES) * sizeof(unsigned long long)));
        HIP_TRY(hipDeviceSynchronize());   // (the fill is on the null stream; the kernels that count may be on any)
        return DAS3R_OK;
    }
    if (g_pairs) {
        HIP_TRY(hipDeviceSynchronize());
        if (out) HIP_TRY(hipMemcpy(out, g_pairs, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIP_TRY(hipFree(g_pairs));
        g_pairs = nullptr;
    } else if (out) {
        out[0] = out[1] = out[2] = out[3] = 0;
    }
    return DAS3R_OK;
}

// Live pairs of a forward (pair_count.hip): out[0] = (pixel, splat) pairs that were blended, out[1] = (pixel, list position) pairs in
// front of the pixels' last contributors (what a walk without any culling would evaluate).  Synchronises the stream; measurement only.
extern "C" int das3r_raster_count_live_pairs(const das3r_raster_args *a, const das3r_raster_saved *saved, uint64_t out[2], das3r_stream_t stream) {
    if (!a || !saved || !out) { set_error("das3r_raster_count_live_pairs: null argument"); return DAS3R_ERR_INVALID_ARG; }
    out[0] = out[1] = 0;
    if (a->P == 0 || saved->num_rendered <= 0) return DAS3R_OK;
    if (!saved->geom || !saved->binning || !saved->img) { set_error("das3r_raster_count_live_pairs: saved buffers missing"); return DAS3R_ERR_INVALID_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const Buffers v = saved_buffers(a, nullptr, saved);
    unsigned long long *dev = nullptr;
    HIP_TRY(hipMalloc((void **)&dev, 2 * sizeof(unsigned long long)));
    int rc = DAS3R_OK;
    if (hipMemsetAsync(dev, 0, 2 * sizeof(unsigned long long), s) != hipSuccess) rc = DAS3R_ERR_HIP;
    if (!rc) rc = launch_count_live_pairs(a, v, dev, s);
    if (!rc && (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(out, dev, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error("das3r_raster_count_live_pairs: device error");
        rc = DAS3R_ERR_HIP;
    }
    (void)hipFree(dev);
    return rc;
}

#ifdef DAS3R_EXPERIMENTS
static unsigned long long *g_trace = nullptr;
namespace das3r { unsigned long long *wg_trace() { return g_trace; } }
// enable != 0: (allocate and) zero the trace, the partition passes stamp from now on; enable == 0: copy it to out (TRACE_PASSES x
// TRACE_WGS x TRACE_STAMPS words) and stop.
extern "C" int das3r_debug_wg_trace(int enable, uint64_t *out) {
    const size_t words = (size_t)TRACE_PASSES * TRACE_WGS * TRACE_STAMPS;
    if (enable) {
        if (!g_trace) HIP_TRY(hipMalloc((void **)&g_trace, words * 8));
        HIP_TRY(hipMemset(g_trace, 0, words * 8));
        HIP_TRY(hipDeviceSynchronize());
        return DAS3R_OK;
    }
    if (g_trace) {
        HIP_TRY(hipDeviceSynchronize());
        if (out) HIP_TRY(hipMemcpy(out, g_trace, words * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipFree(g_trace));
        g_trace = nullptr;
    }
    return DAS3R_OK;
}
// Phase clocks (make EXPERIMENTS=1 only; tools/phase_clocks.py): while the pair counters are on, wave 0 of every workgroup of
// render_forward_rows_kernel / render_backward_blk_kernel adds the shader clocks it spent in each phase of its tile to the words
// behind the pair counters (common.h PHASE_*).  Read them BEFORE das3r_pair_counters(0, ..) frees the array.
extern "C" int das3r_debug_phase_clocks(uint64_t out[16]) {
    for (int i = 0; i < PHASE_WORDS; i++) out[i] = 0;
    if (!g_pairs) return DAS3R_OK;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> all(PHASE_WORDS * PHASE_COPIES);
    HIP_TRY(hipMemcpy(all.data(), g_pairs + 4, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < all.size(); i++) out[i % PHASE_WORDS] += all[i];
    return DAS3R_OK;
}
#endif

// ---- profiling introspection ----
extern "C" void das3r_profile_enable(int on) { g_prof_on = on != 0; }

// Synchronises, then writes one line per kernel name: "<name> <launches> <total_ms>\n"; clears the records.
// Returns the number of bytes written (excluding the terminator) or a negative status.
extern "C" int das3r_profile_report(char *buf, size_t cap) {
    struct Agg { const char *name; int n; double ms; };
    std::vector<Agg> agg;
    for (auto &r : g_prof) {
        float ms = 0.f;
        if (hipEventSynchronize(r.stop) == hipSuccess && hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) {
            bool found = false;
            for (auto &a : agg)
                if (strcmp(a.name, r.name) == 0) { a.n++; a.ms += ms; found = true; break; }
            if (!found) agg.push_back({r.name, 1, (double)ms});
        }
        g_event_pool.push_back(r.start);
        g_event_pool.push_back(r.stop);
    }
    g_prof.clear();
    size_t off = 0;
    for (auto &a : agg) {
        int w = snprintf(buf + off, off < cap ? cap - off : 0, "%s %d %.6f\n", a.name, a.n, a.ms);
        if (w < 0 || off + (size_t)w >= cap) { set_error("das3r_profile_report: buffer too small"); return DAS3R_ERR_INVALID_ARG; }
        off += (size_t)w;
    }
    if (cap) buf[off < cap ? off : cap - 1] = 0;
    return (int)off;
}
