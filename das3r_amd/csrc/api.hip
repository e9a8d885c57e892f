// api.hip — the C-ABI entry points of libdas3r_hip.so (include/das3r_raster.h) and the buffer layout.
#include <stdarg.h>
#include <string.h>

#include <vector>

#include "common.h"
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
// not: every host thread that renders on a device registers there (per_device(), below; un-registered when the thread ends), and
// once a second thread has, every chained kernel of that device takes its tickets — whatever farm.run_jobs or the environment say
// (a DAS3R_TICKETS bound set by hand still wins: it is an experiment switch, and says so once on stderr).  Two PROCESSES on one GPU
// are not seen from here: tools/jobs_per_gpu.py's process mode sets DAS3R_TICKETS=always for its children.
constexpr int MAX_DEVICES = 64;
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

// One side stream and its two events per (host thread, device, caller stream), created at the first split forward of the stream and destroyed
// with the thread.  K jobs in flight (farm.run_jobs: K host threads, each on its own stream) get one each; the hardware queue count is the
// runtime's business.  (A side stream of the lowest priority the device offers measured the same as this one: ledger.)
struct SideStreams {
    struct Entry { int dev; hipStream_t caller; SideStream ss; };
    std::vector<Entry> all;
    ~SideStreams() {
        for (auto &e : all) {
            (void)hipEventDestroy(e.ss.fork);
            (void)hipEventDestroy(e.ss.join);
            (void)hipStreamDestroy(e.ss.stream);
        }
    }
};
static int side_stream_for(hipStream_t s, SideStream *out) {
    static thread_local SideStreams streams;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    for (auto &e : streams.all)
        if (e.dev == dev && e.caller == s) { *out = e.ss; return DAS3R_OK; }
    SideStream ss = {nullptr, nullptr, nullptr, 0};
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    ss.colour_blocks = COLOUR_WGS_PER_CU * (cus > 0 ? cus : 1);
    HIP_TRY(hipStreamCreateWithFlags(&ss.stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&ss.fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ss.join, hipEventDisableTiming));
    streams.all.push_back(SideStreams::Entry{dev, s, ss});
    *out = ss;
    return DAS3R_OK;
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

// Depth histograms of the segmented path (segkey.h), round 6: two 256-word slots per (host thread, device, stream), used in turn.  A forward's
// preprocess kernel accumulates into one and ZEROES THE OTHER for the next forward of the stream — the memset that used to precede every
// forward (a launch of its own: 5 us of every DAS3R-shaped iteration) is gone.  Launches of one stream are ordered, so the slot a forward
// zeroes is read by nobody (the previous forward's emission has finished), and the slot it reads stays as it is until the NEXT forward's
// preprocess kernel, however often its own emission is redone.  Should a slot ever be dirty — an aborted forward — the buckets come out
// less even for one forward and exact all the same: any histogram gives a monotone map, the same one in every workgroup.
static bool dhist_slots(hipStream_t s, uint32_t **use, uint32_t **next) {
    struct Slot { int dev; hipStream_t stream; uint32_t *buf; uint32_t turn; };
    static thread_local std::vector<Slot> slots;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    Slot *e = nullptr;
    for (auto &c : slots)
        if (c.dev == dev && c.stream == s) e = &c;
    if (!e) {
        uint32_t *buf = nullptr;
        if (hipMalloc((void **)&buf, 2 * 256 * sizeof(uint32_t)) != hipSuccess) return false;
        if (hipMemsetAsync(buf, 0, 2 * 256 * sizeof(uint32_t), s) != hipSuccess) return false;   // (on the stream whose kernels use it: ordered)
        slots.push_back(Slot{dev, s, buf, 0u});
        e = &slots.back();
    }
    e->turn++;
    *use = e->buf + 256 * (e->turn & 1u);
    *next = e->buf + 256 * ((e->turn + 1u) & 1u);
    return true;
}
// The depth histogram of this forward (segkey.h): filled by the preprocess kernel, read by the emission.  Not segmented: none (nulls).
// No slot: in the geometry buffer, zeroed by a memset, as before round 6 (*next stays null).
static int seg_dhist_for(bool seg, hipStream_t s, char *geom, const Layout &L, uint32_t **use, uint32_t **next) {
    *use = *next = nullptr;
    if (seg && !dhist_slots(s, use, next)) {
        *use = (uint32_t *)(geom + L.g_dhist);
        HIP_TRY(hipMemsetAsync(*use, 0, 4 * 256, s));
    }
    return DAS3R_OK;
}

static int validate(const das3r_raster_args *a, const das3r_raster_in *in) {
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
    return ForwardPlan{p->local != 0, p->seg != 0, p->seg_bits, p->seg_passes, p->speculate != 0, p->cap, p->decide_fine != 0, p->gen};
}
}  // namespace
extern "C" void das3r_debug_path_policy_fresh(das3r_path_policy_state *state, uint32_t gen) { policy_state_to(Verdict::fresh(gen), Resume(), state); }
extern "C" void das3r_debug_path_policy_plan(das3r_path_policy_state *state, const das3r_path_policy_inputs *in, das3r_path_policy_plan *out) {
    PolicyOnState on(state);
    const ForwardPlan p = plan_forward(on.v, on.inputs(in));
    *out = das3r_path_policy_plan{p.local, p.seg, p.seg_bits, p.seg_passes, p.speculate, p.decide_fine, p.gen, p.cap};
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

extern "C" int das3r_raster_get_layout(int32_t P, int64_t num_rendered, int32_t W, int32_t H, das3r_raster_layout *out) {
    if (!out || P < 0 || num_rendered < 0 || W <= 0 || H <= 0) { set_error("das3r_raster_get_layout: invalid argument"); return DAS3R_ERR_INVALID_ARG; }
    Layout L;
    compute_layout(P, num_rendered, W, H, &L);
    *out = L.pub;
    return DAS3R_OK;
}

// Host mailbox: a pinned, device-visible block per host thread and device.  The scan kernel stores {count, flags} and then the
// tag of the call (system-scope release) into words 0..2; word 10 is raised by a compositing kernel that met a tile list too
// long for its LDS sort; the last binning kernel of a forward stores {self-check word, tag} into one of CHECK_SLOTS two-word
// slots from word 16 on (slot = tag % CHECK_SLOTS).  The host polls the tags — no D2H copy kernel, no event, no parked thread
// (hipEventSynchronize's wake-up alone cost ~100 us per forward, a third of a 100 k-splat step).
struct Mailbox {
    volatile uint32_t *host = nullptr;
    uint32_t *dev = nullptr;
    uint32_t seq = 0;
};
// the words the host reads by index (the kernels are handed pointers: dev + MB_COUNT {count, flags, tag}, dev + MB_TOO_LONG {too long,
// want bits}, dev + MB_LONGEST {longest, tag, crowding})
enum MailboxWord : uint32_t {
    MB_COUNT = 0,       // num_rendered of the forward whose tag is in MB_COUNT_TAG
    MB_COUNT_TAG = 2,
    MB_TOO_LONG = 10,   // != 0: a forward of the shape with that generation number met a list too long for LDS (path_policy.h)
    MB_WANT_BITS = 11,  // != 0: the segmented path of that generation sorted a segment long enough to want more bucket bits
    MB_FILTERED = 12,   // the tag of a forward whose preprocess kernel culled a point
    MB_LONGEST = 13,    // list_skew_kernel: the longest tile list of the forward whose tag is in MB_SKEW_TAG
    MB_SKEW_TAG = 14,
    MB_CROWD16 = 15,    // ... and of 64 consecutive list entries, those in the tile's fullest quadrant, x 16
};
// the tag of the next hand-off through the mailbox (never 0: an empty word names nobody)
static uint32_t next_tag(Mailbox *mb) { return ++mb->seq ? mb->seq : ++mb->seq; }
// Everything the library remembers between calls, per host thread and per device (a thread that renders on two GPUs gets two
// of these; nothing is shared between threads: any number of them may render concurrently, each on its own stream).
constexpr uint32_t CHECK_SLOTS = 16, CHECK_WORD0 = 16, MAILBOX_BYTES = 4 * (CHECK_WORD0 + 2 * CHECK_SLOTS);
struct PerDevice {
    Mailbox mb;
    uint32_t pending[CHECK_SLOTS] = {};             // per slot: tag of the forward whose self-check word has not been examined yet
    unsigned long long *arrive_ring = nullptr;      // self re-arming arrival words of the preprocess kernel's count reduction
    Verdict verdict;                                // what the last forward of the current shape (P, W, H) taught us (path_policy.h)
    Resume resume;                                  // das3r_raster_learning(set): handed to the next shape this thread meets
    char *emit_ring = nullptr;                      // control words of the emission fused into the preprocess kernel
    bool emit_ring_dirty = false;
    uint32_t emit_last_tag = 0;
};
static int per_device(PerDevice **out) {
    static thread_local PerDevice state[MAX_DEVICES];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) { set_error("device ordinal %d not supported", dev); return DAS3R_ERR_INVALID_ARG; }
    PerDevice &T = state[dev];
    g_registrar.add(dev);   // (grid_is_resident: a second rendering thread on the device switches the ticket-free short cut off)
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

// Examine the self-check word a forward's last binning kernel left in `slot` = {flags, tag} of a host mailbox (bit 1 look-back
// timeout, 2 index out of range -> write suppressed, 8 counts do not add up to the histogram; 16 = a stalled look-back was rescued,
// granule.h: informational).  wait: spin (bounded) until the word of `tag` is there.  Returns 1 when the slot does not hold
// `tag`'s word (not there yet, or — after CHECK_SLOTS later forwards, each of which examines the slot before reusing it — gone).
static unsigned long long g_stats[4] = {0, 0, 0, 0};   // forwards, self-check words examined, rescued look-back polls, failed self-checks
static void stat_add(int i) { __atomic_fetch_add(&g_stats[i], 1ull, __ATOMIC_RELAXED); }
static int examine_check_slot(volatile uint32_t *slot, uint32_t tag, bool wait, hipStream_t s) {
    uint32_t seen = __atomic_load_n(&slot[1], __ATOMIC_ACQUIRE);
    if (seen != tag && wait) {
        const int r = await_tag(&slot[1], tag, s, &seen);
        if (r) return r;
    }
    if (seen != tag) return 1;
    const uint32_t all_flags = slot[0], flags = all_flags & ~16u;
    if (all_flags & 0x80000000u) return DAS3R_OK;   // this forward's failure has been reported already (by the backward pass / das3r_raster_check)
    stat_add(1);
    if (all_flags & 16u) stat_add(2);
    if (flags) stat_add(3);
    if ((all_flags & 16u) && switches().verbose) fprintf(stderr, "das3r: a look-back poll needed the read-modify-write path\n");
    if (flags) {
        slot[0] = all_flags | 0x80000000u;   // reported once: the thread that made the forward will not report it again at its next call
        set_error("a forward's binning failed its self-check (flags 0x%x); its output is invalid", flags);
        return DAS3R_ERR_HIP;
    }
    return DAS3R_OK;
}

// The self-check of the forward that produced `saved`, for callers that want it BEFORE they consume the image (the forward
// itself returns as soon as everything is enqueued; das3r_raster_backward runs this first).  Waits, bounded, for the word.
extern "C" int das3r_raster_check(const das3r_raster_saved *saved, das3r_stream_t stream) {
    if (!saved) { set_error("das3r_raster_check: null saved state"); return DAS3R_ERR_INVALID_ARG; }
    if (!saved->check_word || !saved->check_tag) return DAS3R_OK;   // P == 0, nothing rendered, or a caller that dropped the ticket
    const int r = examine_check_slot((volatile uint32_t *)saved->check_word, saved->check_tag, true, (hipStream_t)stream);
    return r < 0 ? r : DAS3R_OK;
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

extern "C" void das3r_get_stats(uint64_t out[4]) {
    for (int i = 0; i < 4; i++) out[i] = (uint64_t)__atomic_load_n(&g_stats[i], __ATOMIC_RELAXED);
}

extern "C" int64_t das3r_raster_forward(const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_out *out,
                                        das3r_alloc_fn alloc_geom, das3r_alloc_fn alloc_binning, das3r_alloc_fn alloc_img,
                                        void *user, das3r_raster_saved *saved, das3r_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    stat_add(0);
    int rc = validate(a, in);
    if (rc) return rc;
    if (!out || !out->out_color || (a->P > 0 && !out->radii) || !alloc_geom || !alloc_binning || !alloc_img || !saved) {
        set_error("das3r_raster_forward: null output/allocator");
        return DAS3R_ERR_INVALID_ARG;
    }
    if (out->out_invdepth && !fwd_has_invdepth_form(switches().render_fwd)) {   // ABI 16: every forward kernel the library picks has an inverse-depth form, not the forced slices
        set_error("das3r_raster_forward: DAS3R_RENDER=%s has no inverse-depth form (das3r_raster_out.out_invdepth)", fwd_kernel_name(switches().render_fwd));
        return DAS3R_ERR_INVALID_ARG;
    }
    const int P = a->P, W = a->image_width, H = a->image_height;
    const bool depth = out->out_invdepth != nullptr;   // ABI 16: the binning buffer also holds Layout::d_* (d_bytes instead of binning_bytes)
    // the geometry buffer also holds Layout::g_shjac (flags bit 2) — unless the caller said that no backward will read it (flags bit 3 on the
    // way in, read before the struct is cleared below)
    const bool shjac = in->shs != nullptr && a->sh_degree >= 2 && !(saved->flags & NO_BACKWARD_IN_FLAG);
    const bool no_backward = (saved->flags & NO_BACKWARD_IN_FLAG) != 0;
    const bool aa = (saved->flags & ANTIALIAS_FLAG) != 0;   // (bit 4 on the way in: an antialiased forward; set again on the way out)
    Layout L;
    compute_layout(P, 0, W, H, &L, shjac);
    saved->geom = alloc_geom(user, L.pub.geom_bytes);
    saved->img = alloc_img(user, L.pub.img_bytes);
    saved->binning = nullptr;
    saved->num_rendered = 0;
    saved->capacity = 0;
    saved->check_word = nullptr;
    saved->check_tag = 0;
    saved->flags = aa ? ANTIALIAS_FLAG : 0u;
    if (!saved->geom || !saved->img) { set_error("scratch allocation failed (geom %zu B, img %zu B)", L.pub.geom_bytes, L.pub.img_bytes); return DAS3R_ERR_ALLOC; }
    if (P == 0) {
        // upstream:rasterize_points.cu skips the rasterizer when P == 0: the image stays zero (background NOT applied)
        HIP_TRY(hipMemsetAsync(out->out_color, 0, sizeof(float) * 3 * (size_t)W * H, s));
        if (out->out_invdepth) HIP_TRY(hipMemsetAsync(out->out_invdepth, 0, sizeof(float) * (size_t)W * H, s));
        HIP_TRY(hipMemsetAsync(saved->img + L.pub.ranges, 0, 8 * (size_t)L.ntiles, s));
        saved->binning = alloc_binning(user, 256);
        return 0;
    }
    // Host <-> device hand-offs of one forward (all through the pinned mailbox, no copies, no events):
    //   * num_rendered (sum of tiles_touched) leaves with the preprocess kernel, five kernels before the device needs it, so
    //     the binning buffer is sized exactly and the host practically never waits (upstream blocks on a cudaMemcpy in the
    //     middle of every forward); on the local-order path nothing waits for it at all (speculative capacity, below);
    //   * the binning self-check word is delivered by the last binning kernel into a slot of the mailbox; saved->check_word /
    //     check_tag name it.  It is examined by das3r_raster_backward (before anything is launched) and das3r_raster_check, which
    //     wait for it, and — for callers that use neither — without waiting at the start of this thread's later forwards;
    //     debug mode waits for it before returning.
    PerDevice *T = nullptr;
    if ((rc = per_device(&T))) return rc;
    Mailbox *mb = &T->mb;
    auto check_slot = [&](uint32_t i, bool wait) -> int {
        if (!T->pending[i]) return DAS3R_OK;
        const int r = examine_check_slot(mb->host + CHECK_WORD0 + 2 * i, T->pending[i], wait, s);
        if (r == 1) return DAS3R_OK;   // not there yet: look again next time
        T->pending[i] = 0;
        return r;
    };
    for (uint32_t i = 0; i < CHECK_SLOTS; i++)
        if ((rc = check_slot(i, false))) return rc;
    uint32_t late_tag = 0;
    // per-thread ring of self re-arming arrival words for the count reduction of the preprocess kernel
    unsigned long long *&arrive_ring = T->arrive_ring;
    constexpr uint32_t ARRIVE_SLOTS = 16, ARRIVE_WORDS = 8 + 64 * 8;   // per call: top word + 64 sub-counters, one 64-byte line each
    if (!arrive_ring) {
        HIP_TRY(hipMalloc((void **)&arrive_ring, ARRIVE_SLOTS * ARRIVE_WORDS * sizeof(unsigned long long)));
        // on the CALLER'S stream, in front of the kernel that counts in it: hipMemset runs on the null stream, which a non-blocking stream
        // does not wait for — with a second job keeping the GPU busy (round 5: farm.run_jobs) the fill could land AFTER the first preprocess
        // kernel of this thread had started counting, the last arriver never saw its total, and the forward ended with "the device never
        // delivered the result of this forward to the host mailbox" (one first-forward in a few dozen two-job runs)
        HIP_TRY(hipMemsetAsync(arrive_ring, 0, ARRIVE_SLOTS * ARRIVE_WORDS * sizeof(unsigned long long), s));
        // ... and COMPLETE before this call goes on: the ring belongs to the thread, not to the stream — the same thread's next forward may
        // be issued on another non-blocking stream, which does not wait for this one.  Once per thread and device.
        HIP_TRY(hipStreamSynchronize(s));
    }
    // Which binning path this forward takes, whether it speculates on its capacity and whether it looks at its tile lists: path_policy.h,
    // from what the earlier forwards of the shape left in T->verdict and the two words their kernels may have raised since.
    const uint32_t too_long = mb->host[MB_TOO_LONG];
    if (too_long) mb->host[MB_TOO_LONG] = 0;
    const uint32_t want_bits = mb->host[MB_WANT_BITS];
    if (want_bits) mb->host[MB_WANT_BITS] = 0;
    const PolicyInputs policy_in = {P, W, H, L.ntiles, L.tbits, L.tile_passes, too_long, want_bits, switches().binning /* DAS3R_BINNING */, use_onesweep(),
                                    a->capacity_hint, switches().capacity_exact, &T->resume};
    const ForwardPlan plan = plan_forward(T->verdict, policy_in);
    bool local = plan.local;
    const bool seg = plan.seg;
    const uint32_t *seg_dhist = nullptr;   // where this forward's depth histogram is (set with the preprocess launch, below)
    auto apply_seg = [&]() {   // (compute_layout starts every layout without buckets)
        L.dhist_ptr = seg_dhist;
        if (seg) {
            L.dbits = plan.seg_bits;
            L.kbits = L.tbits + plan.seg_bits;
            L.kshift = std::min(16, 32 - L.kbits);
            L.part_passes = plan.seg_passes;
        }
    };
    const uint32_t count_tag = next_tag(mb);
    unsigned long long *arrive = arrive_ring + (size_t)(count_tag % ARRIVE_SLOTS) * ARRIVE_WORDS;
    // The split preprocess: the fork event is recorded behind the geometry kernel (launch_preprocess); the colour kernel goes to the side
    // stream once the binning kernels are enqueued on s (join.launch()), and s waits for it (join.now()) in front of the first kernel that
    // reads a colour, `clamped` or a Jacobian plane — the compositing forward.  Whatever is pending on the side stream when this function
    // returns, on EVERY way out, s waits for: once the call's work on s is complete the side stream touches neither the caller's tensors
    // nor the geometry buffer.  (A way out between the fork and the launch leaves nothing on the side stream.)
    struct Join {
        hipStream_t s;
        const das3r_raster_args *a;
        const das3r_raster_in *in;
        char *const *geom;
        const Layout *L;
        SideStream side;
        bool forked, pending;
        int launch() {
            if (!forked) return DAS3R_OK;
            forked = false;
            pending = true;   // (from the first call that touches the side stream on)
            return launch_sh_colour(a, in, *geom, *L, &side);
        }
        int now() {
            const int r = launch();
            if (r) return r;
            if (!pending) return DAS3R_OK;
            pending = false;
            HIP_TRY(hipStreamWaitEvent(s, side.join, 0));
            return DAS3R_OK;
        }
        ~Join() {
            if (pending) (void)hipStreamWaitEvent(s, side.join, 0);
        }
    } join = {s, a, in, &saved->geom, &L, {nullptr, nullptr, nullptr, 0}, false, false};
    auto split_side = [&](int binning_path, const SideStream **side) -> int {   // *side: null = the fused kernel
        *side = nullptr;
        if (!split_colour_rule(in->shs != nullptr, a->sh_degree, P, binning_path, no_backward, switches().split_colour)) return DAS3R_OK;
        const int r = side_stream_for(s, &join.side);
        if (r) return r;
        *side = &join.side;
        return DAS3R_OK;
    };
    // everything behind the count: scan + emission, partition, tile ranges, compositing (L laid out for `cap`, buffer allocated)
    auto bin_and_render = [&](int64_t cap, bool local_order, bool ctrl_zeroed, uint32_t *count_out = nullptr, uint32_t count_out_tag = 0,
                              uint32_t *emit_slot = nullptr /*the preprocess kernel has emitted the instances already*/) -> int {
        int r;
        const bool fused_scan = use_onesweep();   // scan + emission in one kernel; the classic path scans, then emits
        const bool seg = L.dbits > 0;             // segmented path: index-order emission with depth buckets, lists sorted by segment_sort_kernel
        if (!emit_slot) {
            if (fused_scan) {
                if ((r = launch_binning_scan_emit(P, cap, out->radii, saved->geom, saved->binning, L, ctrl_zeroed, count_out, count_out_tag, a->debug != 0,
                                                  s, local_order || seg))) return r;
            } else if ((r = launch_scan(P, saved->geom, L, nullptr, 0, a->debug != 0, s))) return r;
        }
        uint32_t *host_late = nullptr;
        if (cap > 0) {
            late_tag = next_tag(mb);
            const uint32_t slot = late_tag % CHECK_SLOTS;
            if ((r = check_slot(slot, true))) return r;   // (the forward that used the slot CHECK_SLOTS forwards ago)
            T->pending[slot] = late_tag;
            host_late = mb->dev + CHECK_WORD0 + 2 * slot;
            saved->check_word = (void *)(mb->host + CHECK_WORD0 + 2 * slot);
            saved->check_tag = late_tag;
        }
        uint32_t *dead_keys = nullptr;
        if ((r = launch_binning(P, cap, W, H, out->radii, saved->geom, saved->binning, saved->img, L, fused_scan, host_late, late_tag,
                                a->debug != 0, s, &dead_keys, emit_slot, mb->dev + MB_TOO_LONG, plan.gen))) return r;
        if ((r = join.launch())) return r;   // the split preprocess: the colour kernel, beside the binning kernels enqueued above
        LocalBin lb = {(float4 *)(saved->binning + L.b_ckpt), nullptr, nullptr, nullptr, nullptr, plan.gen, (uint32_t)(P - 1), (uint32_t)cap};
        // The three questions below — look at the list skew? order the tiles longest first? leave the backward its hint? — are asked with
        // local_lists = false, "by shape", on every binning path: lb.point_list is only set further down, so that is what these sites have always
        // answered.  launch_render_forward, which sees the pointer, passes the truth, and on the local-order path never takes the lanes /
        // regions kernels the answers here are about; the hint's bit 0 still steers that forward's BACKWARD (kernel_choice.h choose_backward).
        // Kept as it is: changing it changes which kernels a training run takes.
        const bool by_shape = cap > 0 && quad_lanes(switches(), L.ntiles, L.capacity, /*local_lists=*/false);
        if (plan.decide_fine && by_shape) {   // (shapes the one-workgroup-per-tile kernel would take: few tiles, long lists)
            const uint32_t tag = next_tag(mb);
            if ((r = launch_list_skew(saved->img, saved->binning, saved->geom, L, (uint32_t)cap, (uint32_t)(P - 1), mb->dev + MB_LONGEST, tag, a->debug != 0, s))) return r;
            if ((r = mailbox_wait(mb, MB_SKEW_TAG, tag, s))) return r;
            const uint32_t longest = mb->host[MB_LONGEST], crowd16 = mb->host[MB_CROWD16];
            const int64_t mean = skew_mean(T->verdict, cap, L.ntiles);
            const bool now_fine = learn_skew(T->verdict, longest, crowd16, cap, L.ntiles);
            if (switches().verbose) fprintf(stderr, "[das3r] tile lists: longest %lld, mean %lld, %.1f of 64 consecutive entries in one quadrant -> %s kernels\n", (long long)longest,
                                            (long long)mean, crowd16 / 16.0, now_fine ? "2x2-region" : "block");
        }
        const bool fine = prefers_regions(T->verdict);
        lb.prefer_regions = fine;
        lb.tile_order = nullptr;
        if (tile_lpt_wanted(switches(), L.ntiles, L.capacity, /*local_lists=*/false, fine)) {   // longest lists first (kernel_choice.h says why)
            if ((r = launch_tile_lpt(saved->img, L, (uint32_t)cap, a->debug != 0, s))) return r;
            lb.tile_order = (const uint32_t *)(saved->img + L.i_order);
        }
        if (fine && by_shape) saved->flags |= backward_hint(T->verdict, (uint32_t)BUCKET);   // (for the backward pass of this forward: kernel_choice.h choose_backward)
        if (local_order && cap > 0) {
            lb.point_list = (uint32_t *)(saved->binning + L.pub.point_list);
            lb.slot_list = (uint32_t *)(saved->binning + L.b_slot);
            lb.keys = dead_keys;
            lb.host_flag = mb->dev + MB_TOO_LONG;
        }
        if ((r = join.now())) return r;   // (a redo finds the colours there already: nothing is pending the second time)
        return launch_render_forward(a, in->colors_precomp, out->out_color, saved->geom, saved->binning, saved->img, L, lb, s, out->out_invdepth,
                                     depth ? (float4 *)(saved->binning + L.d_ckpt) : nullptr);
    };
    // prefiltered: the caller's promise that no point fails the near-plane cull (upstream traps when one does: auxiliary.h in_frustum);
    // the preprocess kernel leaves this call's tag in mailbox word 12 when one did
    auto prefiltered_ok = [&]() -> int {
        if (!a->prefiltered || mb->host[MB_FILTERED] != count_tag) return DAS3R_OK;
        set_error("Point is filtered although prefiltered is set. This shouldn't happen!");
        return DAS3R_ERR_INVALID_ARG;
    };
    int64_t I, cap;
    // The speculative flow: the binning buffer is laid out for the plan's capacity and the whole forward is enqueued before the host looks
    // at the mailbox (the kernels clamp to the capacity).  Should the scene have grown past it, the binning and the compositing are redone
    // with the exact size.
    if (plan.speculate) {
        cap = plan.cap;
        compute_layout(P, cap, W, H, &L, shjac);
        apply_seg();
        saved->binning = alloc_binning(user, depth ? L.d_bytes : L.pub.binning_bytes);
        if (!saved->binning) { set_error("scratch allocation failed (binning %zu B)", L.pub.binning_bytes); return DAS3R_ERR_ALLOC; }
        // The count is not needed before the end of this call: the preprocess kernel skips its count reduction and the scan
        // delivers it.  When the preprocess grid is resident as a whole (P <= 196 k) the scan and the emission run inside the
        // preprocess kernel itself (EmitArgs, common.h) and the separate scan + emit kernel is not launched at all; their
        // control words live in a library-owned ring slot per forward, zero at rest.  DAS3R_FUSED_EMIT=0 switches that off.
        char *&emit_ring = T->emit_ring;
        bool &emit_ring_dirty = T->emit_ring_dirty;
        uint32_t &emit_last_tag = T->emit_last_tag;
        constexpr size_t EMIT_SLOT_BYTES = sizeof(uint32_t) * EMIT_SLOT_WORDS + sizeof(unsigned long long) * EMIT_STATUS_GRANULES;
        const bool fused_emit = local && grid_is_resident(div_up(P, 256)) && !switches().fused_emit_off;
        uint32_t *emit_slot = nullptr;
        if (fused_emit) {
            if (!emit_ring) {
                HIP_TRY(hipMalloc((void **)&emit_ring, ARRIVE_SLOTS * EMIT_SLOT_BYTES));
                emit_ring_dirty = true;
            }
            if (emit_ring_dirty || count_tag < emit_last_tag) {   // first use, an aborted forward, or the tags wrapped around
                HIP_TRY(hipMemsetAsync(emit_ring, 0, ARRIVE_SLOTS * EMIT_SLOT_BYTES, s));
                emit_ring_dirty = false;
            }
            emit_last_tag = count_tag;
            emit_slot = (uint32_t *)(emit_ring + (size_t)(count_tag % ARRIVE_SLOTS) * EMIT_SLOT_BYTES);
            const EmitArgs em = {(unsigned long long *)(emit_slot + EMIT_SLOT_WORDS), count_tag, emit_slot + 64, emit_slot,
                                 (uint32_t *)(saved->binning + L.b_keyA), (uint32_t *)(saved->binning + L.b_gid_of),
                                 (uint32_t *)(saved->geom + L.g_off_by_gid), (uint32_t)cap, L.tbits, (uint32_t *)(saved->geom + L.g_count), mb->dev};
            emit_ring_dirty = true;   // until the last binning kernel of this forward is enqueued (it re-arms the slot)
            if ((rc = launch_preprocess(a, in, out->radii, saved->geom, saved->img, saved->binning + L.b_ghist, L.b_ctrl_bytes, L, nullptr, mb->dev,
                                        count_tag, s, &em, nullptr, nullptr, aa))) return rc;
            if ((rc = bin_and_render(cap, true, true, nullptr, 0, emit_slot))) return rc;
            emit_ring_dirty = false;
        } else {
            uint32_t *dhist = nullptr, *dhist_next = nullptr;
            if ((rc = seg_dhist_for(seg, s, saved->geom, L, &dhist, &dhist_next))) return rc;
            seg_dhist = dhist;
            apply_seg();
            const SideStream *side = nullptr;
            if ((rc = split_side(1, &side))) return rc;
            if ((rc = launch_preprocess(a, in, out->radii, saved->geom, saved->img, saved->binning + L.b_ghist, L.b_ctrl_bytes, L, nullptr, mb->dev,
                                        count_tag, s, nullptr, dhist, dhist_next, aa, side))) return rc;
            join.forked = side != nullptr;
            if ((rc = bin_and_render(cap, local, true, mb->dev, count_tag))) return rc;
        }
        if ((rc = mailbox_wait(mb, MB_COUNT_TAG, count_tag, s))) return rc;
        if ((rc = prefiltered_ok())) return rc;
        I = (int64_t)mb->host[MB_COUNT];
        if (I > CAPACITY_MAX) { set_error("num_rendered %lld exceeds 2^31", (long long)I); return DAS3R_ERR_OVERFLOW; }
        (void)learn_count(T->verdict, I, policy_in, plan);   // (enqueued already: this forward keeps its path)
        if (I > cap) {
            cap = I;
            compute_layout(P, cap, W, H, &L, shjac);
            saved->binning = alloc_binning(user, depth ? L.d_bytes : L.pub.binning_bytes);
            if (!saved->binning) { set_error("scratch allocation failed (binning %zu B)", L.pub.binning_bytes); return DAS3R_ERR_ALLOC; }
            apply_seg();
            HIP_TRY(hipMemsetAsync(saved->geom + L.g_ghist, 0, L.g_ctrl_bytes, s));          // tickets and look-back words of the scan
            HIP_TRY(hipMemsetAsync(saved->img + L.pub.ranges, 0, 8 * (size_t)L.ntiles, s));
            if ((rc = bin_and_render(cap, local, false))) return rc;
        }
    } else {
        uint32_t *dhist = nullptr, *dhist_next = nullptr;
        if ((rc = seg_dhist_for(seg, s, saved->geom, L, &dhist, &dhist_next))) return rc;
        seg_dhist = dhist;
        const SideStream *side = nullptr;
        if ((rc = split_side((local || seg) ? 1 : 0, &side))) return rc;
        if ((rc = launch_preprocess(a, in, out->radii, saved->geom, saved->img, nullptr, 0, L, arrive, mb->dev, count_tag, s, nullptr, dhist, dhist_next, aa, side))) return rc;
        join.forked = side != nullptr;
        if (!local && !seg && (rc = launch_depth_sort(P, saved->geom, L, 0, nullptr, 0, a->debug != 0, s))) return rc;
        if ((rc = mailbox_wait(mb, MB_COUNT_TAG, count_tag, s))) return rc;    // usually there already: preprocess finished long ago
        if ((rc = prefiltered_ok())) return rc;
        I = cap = (int64_t)mb->host[MB_COUNT];
        if (cap > CAPACITY_MAX) { set_error("num_rendered %lld exceeds 2^31", (long long)cap); return DAS3R_ERR_OVERFLOW; }
        if (learn_count(T->verdict, I, policy_in, plan)) {   // the scene grew: global sort after all
            local = false;
            if ((rc = join.now())) return rc;   // (the sort scatters the depth keys the colour kernel reads)
            if ((rc = launch_depth_sort(P, saved->geom, L, 0, nullptr, 0, a->debug != 0, s))) return rc;
        }
        compute_layout(P, cap, W, H, &L, shjac);
        apply_seg();
        saved->binning = alloc_binning(user, depth ? L.d_bytes : L.pub.binning_bytes);
        if (!saved->binning) { set_error("scratch allocation failed (binning %zu B)", L.pub.binning_bytes); return DAS3R_ERR_ALLOC; }
        if (!local && !seg && (rc = launch_depth_sort(P, saved->geom, L, 1, saved->binning + L.b_ghist, L.b_ctrl_bytes, a->debug != 0, s))) return rc;
        if ((rc = bin_and_render(cap, local, !local && !seg))) return rc;
    }
    if (a->debug && late_tag && (rc = check_slot(late_tag % CHECK_SLOTS, true))) return rc;   // debug: report this forward's self-check word right away
    saved->num_rendered = I;
    saved->capacity = cap;
    if (depth) saved->flags |= DEPTH_SAVED_FLAG;
    if (shjac) saved->flags |= SHJAC_SAVED_FLAG;
    return I;
}

// flags bit 2: the forward left the SH colour's Jacobian for the per-Gaussian backward (Layout::g_shjac), which then reads it instead of
// the SH rows.  Without it (a caller that handed back flags = 0) the backward reads the rows as before.
static bool shjac_saved(const das3r_raster_args *a, const das3r_raster_in *in, const das3r_raster_saved *saved) {
    return (saved->flags & SHJAC_SAVED_FLAG) != 0 && in->shs != nullptr && a->sh_degree >= 2;
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
    int rc = validate(a, in);
    if (rc) return rc;
    const int P = a->P;
    if (P == 0) {
        if (focal) HIP_TRY(hipMemsetAsync(focal->sums, 0, 2 * sizeof(float), s));   // (per_splat has no element)
        return DAS3R_OK;
    }
    if ((rc = backward_validate(who, in, saved, dL_dpix, depth_pass, dL_dinvdepth, g))) return rc;
    if (depth_pass && (rc = refuse_bwd_without_invdepth(who))) return rc;
    // the forward's binning self-check first: nothing is launched on the strength of an invalid image / list
    if ((rc = das3r_raster_check(saved, stream))) return rc;
    Layout L;
    compute_layout(P, saved->capacity > 0 ? saved->capacity : saved->num_rendered, a->image_width, a->image_height, &L, shjac_saved(a, in, saved));
    // scratch = per-instance partial sums [num_rendered, 9]; no accumulator needs zeroing (no atomics anywhere)
    float *partial = g->scratch;
    const float *dz = nullptr;
    bool quad_rows = false;
    if (saved->num_rendered > 0) {
        if (!saved->binning) { set_error("%s: binning buffer missing", who); return DAS3R_ERR_INVALID_ARG; }
        if ((rc = launch_render_backward(a, dL_dpix, saved->geom, saved->binning, saved->img, L, partial, s, &quad_rows, saved->num_rendered, saved->flags))) return rc;
        if (depth_pass) {
            const size_t c = L.capacity > 0 ? (size_t)L.capacity : 1;
            float *partial_depth = (float *)((char *)g->scratch + align_up(c * 9 * sizeof(float) + 16));
            if ((rc = launch_depth_pass_inputs(P, a->image_width * a->image_height, saved->geom, L, saved->binning, dL_dinvdepth, s, a->debug != 0))) return rc;
            Layout Ld = L;   // the depth pass reads its splat records and checkpoints from the binning buffer's depth part
            Ld.pub.xy = L.d_recs;
            Ld.pub.conic_opacity = L.d_recs + 16;
            Ld.pub.rgbd = L.d_recs + 32;
            Ld.b_ckpt = L.d_ckpt;
            das3r_raster_args ad = *a;
            ad.bg = (const float *)(saved->binning + L.d_bg);
            bool quad_rows_d = false;
            if ((rc = launch_render_backward(&ad, (const float *)(saved->binning + L.d_dpix), saved->binning, saved->binning, saved->img, Ld, partial_depth, s,
                                             &quad_rows_d, saved->num_rendered, saved->flags))) return rc;
            float *dzw = (float *)(saved->binning + L.d_dz);
            if ((rc = launch_depth_fold(P, saved->geom, L, partial, partial_depth, dzw, s, a->debug != 0))) return rc;
            dz = dzw;
        }
    }
    const bool aa = (saved->flags & ANTIALIAS_FLAG) != 0;
    // (nothing rendered: tiles_touched is all zero, the kernel reads no row and writes the zeros)
    if (focal && (rc = launch_focal_grad(a, in, saved->geom, L, partial, quad_rows, aa, focal->sums, focal->per_splat, focal->workspace, s))) return rc;
    // (the depth pass's opacity sums were folded into `partial` above: the antialiasing factor's derivative is applied once, to the total)
    return launch_preprocess_backward(a, in, saved->geom, saved->binning, L, g, partial, s, quad_rows, dz, aa);
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
    const size_t c = capacity > 0 ? (size_t)capacity : 1;
    return align_up(c * 9 * sizeof(float) + 16) + c * 9 * sizeof(float) + 16;
}

// One 36-byte row of partial sums per instance + 16 bytes (the per-Gaussian backward reads the rows of a workgroup as 16-byte
// words up to the boundary above the last row).  (The experimental stream kernel — EXPERIMENTS=1 builds, DAS3R_RENDER_BWD=stream —
// needs up to four 48-byte rows per instance: only then is the larger figure returned.)
extern "C" size_t das3r_raster_backward_scratch_bytes(int64_t capacity) {
    const size_t c = capacity > 0 ? (size_t)capacity : 1;
#ifdef DAS3R_EXPERIMENTS
    if (switches().render_bwd == BWD_STREAM) return std::max(c * 9 * sizeof(float) + 16, stream_scratch_bytes(capacity));
#endif
    return c * 9 * sizeof(float) + 16;
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
    Layout L;
    compute_layout(P, saved->capacity > 0 ? saved->capacity : saved->num_rendered, W, H, &L);
    return launch_render_aux_forward(P, W, H, C, features, out, saved->geom, saved->binning, saved->img, L, saved->num_rendered, a->debug != 0, s);
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
    Layout L;
    compute_layout(P, saved->capacity > 0 ? saved->capacity : saved->num_rendered, W, H, &L);
    return launch_render_aux_adjoint(P, W, H, C, dL_dout, dL_dfeat, accumulate != 0, scratch, saved->geom, saved->binning, saved->img, L, saved->num_rendered, a->debug != 0, s);
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
    Layout L;
    compute_layout(a->P, saved->capacity > 0 ? saved->capacity : saved->num_rendered, a->image_width, a->image_height, &L);
    unsigned long long *dev = nullptr;
    HIP_TRY(hipMalloc((void **)&dev, 2 * sizeof(unsigned long long)));
    int rc = DAS3R_OK;
    if (hipMemsetAsync(dev, 0, 2 * sizeof(unsigned long long), s) != hipSuccess) rc = DAS3R_ERR_HIP;
    if (!rc) rc = launch_count_live_pairs(a, saved->geom, saved->binning, saved->img, L, dev, s);
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
