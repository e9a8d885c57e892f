// kernel_choice.h — the experiment / diagnostic switches (what every DAS3R_* spelling means) and which COMPOSITING kernel a forward and a
// backward launch: the named kinds, the parser, the measured thresholds.  The other half of what a launch is — the binning path — is
// path_policy.h.  Pure host arithmetic: no HIP, no switches(), no error reporting — api.hip parses the environment through parse_switches,
// render_fwd.hip / render_bwd.hip launch what choose_forward / choose_backward say.  Compiles with a plain C++17 compiler
// (das3r_debug_parse_switches / das3r_debug_choose_*: the CPU tests drive every spelling and threshold, tests/test_kernel_choice_host.py).
// A spelling or a threshold is defined HERE and nowhere else: the two kernels of a pair differ in the last bit of T, so a change in this file
// changes what a training run computes.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace das3r {

// The numeric values are quoted by tools and notes in the tree: they stay.
enum FwdKernel : int {
    FWD_AUTO = 0,      // by list length and tile count (choose_forward)
    FWD_QUAD = 1,      // DAS3R_RENDER=quad: a wave per 8x8 quadrant, a pixel per lane (render_fwd.hip)
    FWD_ROWS = 2,      // rows: a 4x4 block per DPP row (render_rows.hip)
    FWD_LANES = 3,     // lanes: four lanes per pixel, one workgroup per tile (render_lanes.hip)
    FWD_SLICES = 4,    // slices: a block's list cut into chunks any wave takes (render_slices.hip; no inverse-depth form)
    FWD_REGIONS = 5,   // fine: sixteen lanes per pixel, a wave per 2x2 region, four workgroups per tile (render_regions.hip)
};
enum BwdKernel : int {
    BWD_AUTO = 0,      // by list length and the forward's hint (choose_backward)
    BWD_DPP = 1,       // DAS3R_RENDER_BWD=dpp: pixel per lane (render_bwd.hip)
    BWD_MFMA = 2,      // mfma: superseded, experiments build only (render_bwd_mfma.hip)
    BWD_SCAN = 3,      // scan[a][<entries per round>]: the quadrant walk on the matrix cores (render_bwd_scan.hip)
    BWD_STREAM = 5,    // stream: experimental, experiments build only (render_bwd_stream.hip)
    BWD_BLK = 6,       // blk[<entries per round>][p<0|1|2>][o<4|5>]: the block walk (render_bwd_blk.hip)
    BWD_REGIONS = 7,   // fine[<entries per round>][q|s]: the 2x2-region walk (render_bwd_rgn.hip)
};
// The A-B forms of the region walk that take a tile in strips (render_bwd_rgn.hip, 128 entries per round only)
enum RegionStrips : int {
    STRIPS_NONE = 0,
    STRIPS_QUADRANT = 1,      // fine...q: a wave per quadrant
    STRIPS_INTERLEAVED = 2,   // fine...s: interleaved
};

static inline const char *fwd_kernel_name(FwdKernel k) {
    switch (k) {
        case FWD_QUAD: return "quad";
        case FWD_ROWS: return "rows";
        case FWD_LANES: return "lanes";
        case FWD_SLICES: return "slices";
        case FWD_REGIONS: return "fine";
        default: return "auto";
    }
}
static inline const char *bwd_kernel_name(BwdKernel k) {
    switch (k) {
        case BWD_DPP: return "dpp";
        case BWD_MFMA: return "mfma";
        case BWD_SCAN: return "scan";
        case BWD_STREAM: return "stream";
        case BWD_BLK: return "blk";
        case BWD_REGIONS: return "fine";
        default: return "auto";
    }
}
// ABI 16: every compositing kernel the library picks by itself has an inverse-depth form; of the forced ones these do not
static inline bool fwd_has_invdepth_form(FwdKernel k) { return k != FWD_SLICES; }
static inline bool bwd_has_invdepth_form(BwdKernel k) { return k != BWD_MFMA && k != BWD_SCAN && k != BWD_STREAM; }

// Experiment / diagnostic switches, read from the environment ONCE — at the first call into the library and
// again whenever das3r_reload_switches() is called (tests and tools flip them between calls) — not on every launch.
struct Switches {
    int sort_ipl;          // DAS3R_SORT_IPL = 4 | 8 | 16: keys per lane of the radix passes (0: by size)
    bool sort_classic;     // DAS3R_SORT=classic: histogram + row scan + scatter per digit instead of the one-sweep passes
    bool rect_upstream;    // DAS3R_RECT=upstream: bin over upstream's 3-sigma square (bit-exact list tests)
    bool verbose;          // DAS3R_VERBOSE
    int binning;           // DAS3R_BINNING=local | radix | seg | seg3 | bucket | cells: 1 | -1 | 2 | 3 | 4 | 5 (0: chosen per scene; seg3 = seg with one more partition pass of
                           // bucket bits; bucket = segmented emission, lists finished by the compositing kernel: path_policy.h bucket_local_rule;
                           // cells = the same, partitioned by reserved ranges and finished per cell: cells_rule)
    bool capacity_exact;   // DAS3R_CAPACITY=exact: never lay the binning buffer out speculatively
    bool fused_emit_off;   // DAS3R_FUSED_EMIT=0
    bool no_sh_stage;      // DAS3R_NO_SH_STAGE
    FwdKernel render_fwd;  // DAS3R_RENDER=quad | rows | lanes | slices | fine (unset: FWD_AUTO)
    BwdKernel render_bwd;  // DAS3R_RENDER_BWD=dpp | mfma | scan... | stream | blk... | fine... (unset: BWD_AUTO)
    int render_bwd_mb;     // scan64 / scan128 / scan256, blk64 / blk128 / blk256, fine96 / fine128 ...: entries per round (0: not given by a spelling)
    bool render_bwd_atomic;   // scana256 / scana512: the quadrant walk with the atomic flush
    int tile_chunk;        // DAS3R_TILE_CHUNK: tiles per chunk of the XCD round robin (render_common.h); -1 = default, 0 = contiguous eighths
    int scan_items;        // DAS3R_SCAN_ITEMS = 1 | 2 | 4 | 8 | 16: ranks per thread of the scan + emission kernel (0: by size)
    bool deterministic;    // DAS3R_DETERMINISTIC=1: bit-identical gradients run to run (the block-walk backward for every list length:
                           // the pixel-per-lane kernel meets its four waves with LDS float atomics, whose order varies)
    int render_bwd_occ;    // blk...o<4|5>: workgroups per CU the kernel is compiled for (register cap)
    bool tile_lpt_off;     // DAS3R_TILE_LPT=0
    int render_bwd_pix;    // blk...p<0|1|2>: where render_bwd_blk.hip keeps the per-pixel values (render_blk.h)
    RegionStrips render_bwd_strips;   // fine...q / fine...s: the strip forms of the region walk
    bool bwd_reduce_set, bwd_reduce_shfl;   // DAS3R_BWD_REDUCE=shfl | dpp (reference reduction of the pixel-per-lane kernel)
    bool ablate_set;       // DAS3R_ABLATE (perf experiments on the pixel-per-lane kernel)
    int ablate;
    int tickets;           // DAS3R_TICKETS=always | never | <bound>: 0 | 1 << 30 | bound (-1: from the device's CU count)
    int bwd_pad_lds, fwd_pad_lds;   // DAS3R_BWD_PAD_LDS / DAS3R_FWD_PAD_LDS: extra dynamic LDS (occupancy experiments)
    int bwd_buckets;       // DAS3R_BWD_BUCKETS=0 | <slices>: bucket-parallel backward off / forced with that many slices (-1: by list length)
    int inject_fault;      // das3r_debug_inject_fault (not an environment variable): bits OR-ed into the binning self-check word of every forward (fault-injection tests)
    int mutate;            // das3r_debug_mutate (tests): 1 = the block-walk backward evaluates exp(power) (1 + 1e-4) — a biased kernel the parity tests must catch
    bool fwd_no_prefetch;  // DAS3R_FWD_PREFETCH=0: the rows forward kernel without its software prefetch (A-B runs)
    int split_colour;      // DAS3R_SPLIT_COLOUR=0 | 1: the split preprocess (preprocess.hip) forced off (-1) / on (1) where it can run; unset (0): by shape (forward.hip split_colour_rule)
    int tile_strip;        // DAS3R_TILE_STRIP: rows per strip of the compositing kernels' tile order (0 = row-major)
};

// `lookup`: const char *(const char *name) — a variable's value, or null; an empty string counts as unset (but for DAS3R_NO_SH_STAGE, whose
// presence alone is the switch).  Matching is by first letter unless said otherwise: DAS3R_RENDER_BWD=s... is `scan` unless it starts with
// "stream"; a number in a spelling is the first run of digits in it; the suffixes of blk / fine are looked for anywhere in the spelling.
// Switches that select between CORRECT code paths (tests force each of them) are read in every build.  Those that exist for
// timing experiments only — some of them produce wrong results by design (DAS3R_ABLATE) — are read only with `experiments`
// (make EXPERIMENTS=1): a stray environment variable cannot change what the shipped library computes.  Fault injection
// for the self-check tests is a call (das3r_debug_inject_fault), not an environment variable: inject_fault and mutate stay 0 here.
template <class Lookup>
static inline Switches parse_switches(Lookup &&lookup, bool experiments) {
    Switches w;
    memset(&w, 0, sizeof(w));
    auto env = [&](const char *k) -> const char * { const char *e = lookup(k); return (e && e[0]) ? e : nullptr; };
    auto number_in = [](const char *e, int none) {   // the first run of digits of a spelling
        while (*e && (*e < '0' || *e > '9')) e++;
        return *e ? atoi(e) : none;
    };
    const char *e;
    if (experiments) {
        if ((e = env("DAS3R_SORT_IPL"))) { const int v = atoi(e); w.sort_ipl = (v == 4 || v == 8 || v == 16) ? v : 0; }
        w.sort_classic = (e = env("DAS3R_SORT")) && e[0] == 'c';
        w.no_sh_stage = lookup("DAS3R_NO_SH_STAGE") != nullptr;
        if ((e = env("DAS3R_ABLATE"))) { w.ablate_set = true; w.ablate = atoi(e); }
        if ((e = env("DAS3R_BWD_PAD_LDS"))) w.bwd_pad_lds = atoi(e);
        if ((e = env("DAS3R_FWD_PAD_LDS"))) w.fwd_pad_lds = atoi(e);
        if ((e = env("DAS3R_SCAN_ITEMS"))) { const int v = atoi(e); w.scan_items = (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) ? v : 0; }
        w.fwd_no_prefetch = (e = env("DAS3R_FWD_PREFETCH")) && e[0] == '0';
    }
    w.rect_upstream = (e = env("DAS3R_RECT")) && e[0] == 'u';
    w.verbose = env("DAS3R_VERBOSE") != nullptr;
    if ((e = env("DAS3R_BINNING"))) w.binning = e[0] == 'l' ? 1 : (e[0] == 'r' ? -1 : (e[0] == 's' ? (strchr(e, '3') ? 3 : 2) : (e[0] == 'b' ? 4 : (e[0] == 'c' ? 5 : 0))));
    w.capacity_exact = (e = env("DAS3R_CAPACITY")) && e[0] == 'e';
    w.fused_emit_off = (e = env("DAS3R_FUSED_EMIT")) && e[0] == '0';
    if ((e = env("DAS3R_SPLIT_COLOUR"))) w.split_colour = e[0] == '0' ? -1 : (e[0] == '1' ? 1 : 0);   // (A-B runs, tests: the split preprocess off / on)
    w.tile_lpt_off = (e = env("DAS3R_TILE_LPT")) && e[0] == '0';   // (A-B runs: the region forward in the locality order of the other kernels)
    if ((e = env("DAS3R_RENDER")))
        w.render_fwd = e[0] == 'q' ? FWD_QUAD : (e[0] == 'r' ? FWD_ROWS : (e[0] == 'l' ? FWD_LANES : (e[0] == 's' ? FWD_SLICES : (e[0] == 'f' ? FWD_REGIONS : FWD_AUTO))));
    if ((e = env("DAS3R_RENDER_BWD"))) {
        w.render_bwd = e[0] == 'd' ? BWD_DPP
                     : e[0] == 'm' ? BWD_MFMA
                     : strncmp(e, "stream", 6) == 0 ? BWD_STREAM
                     : e[0] == 's' ? BWD_SCAN
                     : e[0] == 'b' ? BWD_BLK
                     : e[0] == 'f' ? BWD_REGIONS : BWD_AUTO;
        if (w.render_bwd == BWD_BLK) {   // blk<entries per round>[p<PIX>][o<workgroups per CU>]
            w.render_bwd_mb = number_in(e, 128);
            const char *pp = strchr(e, 'p');
            w.render_bwd_pix = pp ? atoi(pp + 1) : 0;
            const char *po = strchr(e, 'o');
            w.render_bwd_occ = po ? atoi(po + 1) : 5;
        }
        if (w.render_bwd == BWD_REGIONS) {   // fine[<entries per round>][q|s]
            w.render_bwd_mb = number_in(e, 128);
            w.render_bwd_strips = strchr(e, 'q') ? STRIPS_QUADRANT : (strchr(e, 's') ? STRIPS_INTERLEAVED : STRIPS_NONE);
        }
        if (w.render_bwd == BWD_SCAN) {   // scan[a][64|128|256|512]
            w.render_bwd_mb = number_in(e, 256);
            // (>= 1000: what the spelling's old encoding, 1000 + entries, made of scan1000 and up; kept)
            w.render_bwd_atomic = strncmp(e, "scana", 5) == 0 || w.render_bwd_mb >= 1000;
        }
    }
    if ((e = env("DAS3R_BWD_REDUCE"))) { w.bwd_reduce_set = true; w.bwd_reduce_shfl = e[0] == 's'; }
    w.tickets = -1;
    if ((e = env("DAS3R_TICKETS"))) w.tickets = e[0] == 'a' ? 0 : (e[0] == 'n' ? 1 << 30 : ((e[0] >= '1' && e[0] <= '9') ? atoi(e) : -1));
    w.deterministic = (e = env("DAS3R_DETERMINISTIC")) && e[0] != '0';
    w.bwd_buckets = -1;
    if ((e = env("DAS3R_BWD_BUCKETS"))) w.bwd_buckets = atoi(e);
    w.tile_strip = 8;
    w.tile_chunk = -1;
    if ((e = env("DAS3R_TILE_CHUNK"))) { const int v = atoi(e); w.tile_chunk = (v >= 0 && v <= 64 && (v & (v - 1)) == 0) ? v : -1; }
    if ((e = env("DAS3R_TILE_STRIP"))) w.tile_strip = std::max(0, std::min(63, atoi(e)));   // (7-bit field of render_common.h pack_tiles, kept below its sign bit)
    return w;
}

// ---- the forward compositing kernel ----
constexpr int64_t ROWS_MEAN_LIST = 128;     // mean list from which the 4x4-block-per-row kernel is taken
constexpr int64_t LANES_MEAN_LIST = 1024;   // ... and from which, with few tiles, the kernels with several lanes per pixel are
constexpr int FEW_TILES = 1024;             // "few tiles": fewer workgroups than the chip has slots for (lanes / regions forward, region-walk backward, tile order)

// Few tiles (fewer waves than the SIMDs can interleave with one pixel per lane), lists from the global sort: the kernels with four / sixteen
// lanes per pixel (render_lanes.hip says why).  local_lists: the tile lists are in index order (local depth order): render_fwd.hip /
// render_rows.hip sort them themselves, the other kernels cannot.
static inline bool quad_lanes(const Switches &sw, int ntiles, int64_t capacity, bool local_lists) {
    if (local_lists) return false;
    if (sw.render_fwd != FWD_AUTO) return sw.render_fwd >= FWD_LANES;
    return ntiles <= FEW_TILES && capacity >= LANES_MEAN_LIST * ntiles;
}
// The row lists cost ~200 instructions per wave and batch to build: worth it once a tile's list is long.  DAS3R_RENDER=quad /
// rows forces one of the two forward kernels (A-B runs, tests); lanes and beyond: those where they apply, else by length.
static inline bool row_private(const Switches &sw, int64_t instances, int ntiles) {
    if (sw.render_fwd == FWD_QUAD || sw.render_fwd == FWD_ROWS) return sw.render_fwd == FWD_ROWS;
    return instances >= ROWS_MEAN_LIST * ntiles;
}
// prefer_regions: the forwards before this one found the shape's tile lists skewed or crowded (path_policy.h Verdict::fine).  Never FWD_AUTO.
static inline FwdKernel choose_forward(const Switches &sw, int ntiles, int64_t capacity, bool local_lists, bool prefer_regions) {
    if (quad_lanes(sw, ntiles, capacity, local_lists)) {
        // one workgroup per tile (lanes), or four (regions) where the tile lists are skewed
        if (sw.render_fwd == FWD_SLICES) return FWD_SLICES;
        if (sw.render_fwd == FWD_REGIONS || (sw.render_fwd == FWD_AUTO && prefer_regions)) return FWD_REGIONS;
        return FWD_LANES;
    }
    return row_private(sw, capacity, ntiles) ? FWD_ROWS : FWD_QUAD;
}
// The region forward takes its tiles longest list first (render_regions.hip tile_lpt_kernel): four workgroups per tile are 3 - 4 generations
// of workgroups on the chip, and a tile whose list is four times the mean (every real sequence has them) that starts in the last generation
// adds its whole chain to the kernel.  DAS3R_TILE_LPT=0: the locality order of the other kernels (A-B runs).
static inline bool tile_lpt_wanted(const Switches &sw, int ntiles, int64_t capacity, bool local_lists, bool prefer_regions) {
    return prefer_regions && capacity > 0 && quad_lanes(sw, ntiles, capacity, local_lists) && ntiles <= FEW_TILES && !sw.tile_lpt_off &&
           (sw.render_fwd == FWD_AUTO || sw.render_fwd == FWD_REGIONS);
}

// ---- the backward compositing kernel ----
// Long tile lists are cut into BUCKETs of list positions: the forward compositing kernels leave every pixel's (T, C) at the bucket
// boundaries in the binning buffer (checkpoints: render_common.h), so that the backward pass can replay the buckets of a tile
// in parallel workgroups (render_bwd_scan.hip) — the DAS3R shape has 416 tiles with ~14 k entries each: one workgroup per tile
// leaves the chip at 1.6 waves per SIMD.
constexpr int BUCKET = 1024;
constexpr int64_t BLK_MEAN_LIST = 96;        // mean list from which the block walk is ahead of the pixel-per-lane kernel
constexpr int64_t LONG_MEAN_LIST = 1024;     // ... from which it takes 192-entry rounds, and the region walk may replace it
constexpr int MAX_SLICES = 32, MAX_HINT_SLICES = 64;   // workgroups per tile of the bucket-parallel replay: by the mean list / by the forward's hint
constexpr int MAX_BUCKET_MB = 256;           // entries per round up to which the kernels have a bucket-parallel form

struct BwdChoice {
    BwdKernel kernel;   // never BWD_AUTO
    int mb;             // entries per round
    int slices;         // > 1: bucket-parallel replay with that many workgroups per tile (scan, blk, regions)
    int pix, occ;       // blk: where the per-pixel values live (render_blk.h), workgroups per CU the kernel is compiled for
    RegionStrips strips;   // regions: the strip forms
    bool atomic_flush;     // scan: the atomic flush
};

// Which decomposition (DAS3R_RENDER_BWD forces one; measurements: DESIGN.md §4):
//   dpp     pixel per lane, cross-lane reduction on the vector ALU (render_bwd.hip): lists of a few hundred entries per tile
//   fine    every DPP row of a wave on a 2x2 region's list, four pixel steps per batch (render_bwd_rgn.hip): long, spatially coherent lists
//   blk     every DPP row of a wave on its own 4x4 block: lanes = 16 splats of the block's culled list, time = its 16 pixels,
//           recurrences as DPP row scans, sums in fp32 registers (render_bwd_blk.hip): everything but short lists
//   scan    lanes = 4 pixels x 16 splats of the QUADRANT's list, sums as split-bf16 products on the matrix cores
//           (render_bwd_scan.hip): round 2's kernel for long lists, kept as the reference for blk
//   stream  the same arithmetic, every wave streaming the tile's list on its own (render_bwd_stream.hip; experimental)
//   mfma    pixel per lane + LDS-transposed slab -> fp32 matrix cores (render_bwd_mfma.hip; superseded by scan)
// num_rendered: the forward's COUNT, not its capacity: the same scene takes the same kernel however its buffer was sized.
// fwd_flags: das3r_raster_saved.flags (bit 0 and bits 8 - 15: path_policy.h backward_hint).
static inline BwdChoice choose_backward(const Switches &sw, int64_t num_rendered, int ntiles, uint32_t fwd_flags) {
    BwdKernel kind = sw.render_bwd;
    int mb = sw.render_bwd_mb ? sw.render_bwd_mb : 256;
    const int64_t tiles = std::max(ntiles, 1);
    if (kind == BWD_AUTO) {
        // measured (render backward, ms; tools/gpu_perf.py): 100 k splats at 1080p, mean list 32: dpp 0.071 / blk64 0.068 / scan128 0.129;
        // 1 M splats, mean 320: dpp 0.532 / scan128 0.476 / blk128p1 0.381; DAS3R shape (13 800, bucket-parallel): dpp 1.89 / scan128 0.78 /
        // blk192 0.497.  Round 2's crossover between dpp and the quadrant walk was a mean list of 192; the block walk culls per 4x4
        // block and is ahead from ~100 entries per tile on (tools/gpu_perf.py --workloads c4:<P>: DESIGN.md section 5).
        const int64_t mean_list = num_rendered / tiles;
        const bool long_lists = mean_list >= BLK_MEAN_LIST;
        kind = (sw.bwd_reduce_set || sw.ablate_set || !long_lists) ? BWD_DPP : BWD_BLK;
        mb = mean_list >= LONG_MEAN_LIST ? 192 : 128;
        // round 6: long lists that the forward found spatially coherent or skewed (das3r_raster_saved.flags bit 0: the depth maps of a real
        // sequence) take the 2x2-region walk — self-consistent Sintel-shaped job: backward 0.548 -> 0.414 ms, dsc 0.865 -> 0.590; random depths
        // stay on the block walk (ds 0.50 against 0.55, noise-depth train step 0.344 against 0.369)
        if (kind == BWD_BLK && mean_list >= LONG_MEAN_LIST && ntiles <= FEW_TILES && (fwd_flags & 1u) && !sw.ablate_set) {
            kind = BWD_REGIONS;
            mb = 128;
        }
        if (sw.deterministic && kind == BWD_DPP) {   // short lists too on the block walk: every sum has a fixed order (rows 0..3 of a wave, waves 0..3)
            kind = BWD_BLK;
            mb = 64;
        }
    }
    BwdChoice c = {kind, mb, 1, 0, 5, STRIPS_NONE, false};
    if (kind == BWD_SCAN || kind == BWD_BLK || kind == BWD_REGIONS) {
        // long lists are replayed bucket by bucket in parallel workgroups (checkpoints from the forward: BUCKET); slices =
        // buckets of an average tile, so that a tile's workgroups take about one bucket each
        int slices = sw.bwd_buckets;
        if (slices < 0) slices = (int)std::min<int64_t>(MAX_SLICES, std::max<int64_t>(1, num_rendered / ((int64_t)BUCKET * tiles)));
        c.atomic_flush = kind == BWD_SCAN && sw.render_bwd_atomic;
        if (slices > 1 && (mb > MAX_BUCKET_MB || c.atomic_flush)) slices = 1;
        // round 6: skewed lists (das3r_raster_saved.flags bits 8 - 15: buckets of the longest list the forward last measured) — a workgroup per
        // bucket of the LONGEST tile; the workgroups of shorter tiles that have no bucket leave before they load anything
        const int hint = (int)((fwd_flags >> 8) & 0xFFu);
        if (sw.bwd_buckets < 0 && kind == BWD_REGIONS && slices > 1 && hint > slices) slices = std::min(hint, MAX_HINT_SLICES);
        c.slices = slices;
    }
    // blk, default (no DAS3R_RENDER_BWD): constants in LDS for 128-entry rounds (1 M splats at 1080p: 0.381 vs 0.407 ms), registers for 192
    // (DAS3R shape: 0.497 vs 0.534 ms)
    c.pix = sw.render_bwd == BWD_BLK ? sw.render_bwd_pix : (mb == 128 ? 1 : 0);
    c.occ = sw.render_bwd_occ == 4 ? 4 : 5;
    if (sw.render_bwd == BWD_REGIONS) c.strips = sw.render_bwd_strips;
    return c;
}

// Switches as a plain struct of integers with the same field names, less inject_fault / mutate (das3r_switches, include/das3r_raster.h)
#define DAS3R_SWITCH_FIELDS(X)                                                                                                              \
    X(sort_ipl) X(sort_classic) X(rect_upstream) X(verbose) X(binning) X(capacity_exact) X(fused_emit_off) X(no_sh_stage) X(render_bwd_mb) \
    X(render_bwd_atomic) X(tile_chunk) X(scan_items) X(deterministic) X(render_bwd_occ) X(tile_lpt_off) X(render_bwd_pix) X(bwd_reduce_set) \
    X(bwd_reduce_shfl) X(ablate_set) X(ablate) X(tickets) X(bwd_pad_lds) X(fwd_pad_lds) X(bwd_buckets) X(fwd_no_prefetch) X(split_colour)   \
    X(tile_strip)
template <class S>
static inline Switches switches_from(const S &s) {
    Switches w;
    memset(&w, 0, sizeof(w));
#define X(f) w.f = static_cast<decltype(w.f)>(s.f);
    DAS3R_SWITCH_FIELDS(X)
#undef X
    w.render_fwd = static_cast<FwdKernel>(s.render_fwd);
    w.render_bwd = static_cast<BwdKernel>(s.render_bwd);
    w.render_bwd_strips = static_cast<RegionStrips>(s.render_bwd_strips);
    return w;
}
template <class S>
static inline void switches_to(const Switches &w, S *s) {
#define X(f) s->f = static_cast<int32_t>(w.f);
    DAS3R_SWITCH_FIELDS(X)
#undef X
    s->render_fwd = w.render_fwd;
    s->render_bwd = w.render_bwd;
    s->render_bwd_strips = w.render_bwd_strips;
}
#undef DAS3R_SWITCH_FIELDS

}  // namespace das3r
