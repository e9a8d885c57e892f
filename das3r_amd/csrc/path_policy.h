// path_policy.h — what a forward LEARNS about a shape (P, W, H) and what the next forward of the shape does with it: which binning path it
// takes (local order, segmented with N partition passes, segmented emission with the local finish — partitioned by the stable passes or by cells —, global radix sort), when a shape backs off to the global sort and for how
// long, whether it speculates on its capacity, and which compositing kernels its tile lists call for.  Pure host arithmetic on a
// caller-owned Verdict: no HIP, no switches(), no error reporting — forward.hip (das3r_raster_forward) reads the mailbox words and the
// switches, calls in here at the places named below, and launches what the plan says.  Compiles with a plain C++17 compiler
// (das3r_debug_path_policy_*: the CPU tests drive every transition through it, tests/test_path_policy_host.py).
#pragma once
#include <stdint.h>

#include <algorithm>

namespace das3r {

constexpr int64_t LOCAL_AVG = 384;            // mean list length up to which the local order wins (measured: 1 M splats at 1080p, mean 320: -4 %)
constexpr int64_t SEG_AVG = 384;              // mean entries per segment up to which the segmented path is taken
constexpr int64_t BUCKET_LOCAL_AVG = 256;     // mean list length ABOVE which (up to LOCAL_AVG) the local order takes its lists pre-ordered by depth bucket (bucket_local_rule)
constexpr int BUCKET_LOCAL_TILES = 1024;      // ... on images of more tiles than this (the lanes / regions shapes keep their paths)
constexpr int BUCKET_LOCAL_DBITS = 2;         // ... when the tile partition's passes have at least this many free key bits
constexpr uint32_t CROWDED16 = 23u * 16u;     // of 64 consecutive list entries, those in the tile's fullest quadrant, x 16, from which a shape is "crowded" (learn_skew)
constexpr uint32_t FINE_PERIOD = 512;         // forwards of a shape between two looks at its tile lists (a power of two: plan_forward)
constexpr int BACKOFF_MIN = 64, BACKOFF_MAX = 4096;   // forwards on the global sort after a failure: doubled from MIN while failures come soon, up to MAX
constexpr uint32_t CLEAN_RESET = 256;         // clean fast-path forwards after which a failure counts as an occasional one (back to BACKOFF_MIN)
constexpr int64_t CAPACITY_MAX = 0x7FFFFF00;  // instances a binning buffer is laid out for at most (forward.hip refuses a larger count: DAS3R_ERR_OVERFLOW)

// depth-bucket bits `passes` partition passes (at most three) have room for beside `tbits` bits of tile id (<= 0: none)
static inline int seg_dbits(int tbits, int passes) { return 8 * (passes < 3 ? passes : 3) - tbits; }

// Every decision of plan_forward starts a new GENERATION of the shape (below); 0 names nobody, so the counter skips it when it wraps.
static inline uint32_t next_gen(uint32_t gen) { return gen + 1u ? gen + 1u : 1u; }

// The fourth binning plan: segmented emission, local finish.  The instances are emitted and partitioned as on the segmented path
// (key = tile << (dbits + fbits) | depth bucket << fbits | fraction: segkey.h, in the passes the tile ids need anyway), but no
// segment_sort_kernel follows: the lists reach the compositing kernel ordered by depth bucket, and its prologue finishes a list of 257 - 512
// entries by ranking every entry inside its (tile, bucket) segment on the fraction bits of the key words (render_common.h
// local_order_tile) instead of gathering depths and running a sort network.  Every other list length takes the local order's branches,
// which are exact whatever the arrival order.  From the call's shape alone: onesweep binning, free key bits, more than 1024 tiles, and the
// learnt mean list in (BUCKET_LOCAL_AVG, LOCAL_AVG] — at or below 256 the rank sort fused with the staging takes nearly every list, and it
// neither needs nor uses the arrival order (the bucket map of the emission would buy nothing).  forced: DAS3R_BINNING=bucket (4) wherever
// the key bits are there.
static inline bool bucket_local_rule(int forced, bool onesweep, int tbits, int tile_passes, int ntiles, int64_t last_I, int radix_left) {
    if (!onesweep || seg_dbits(tbits, tile_passes) < BUCKET_LOCAL_DBITS) return false;
    if (forced == 4 || forced == 5) return true;
    return forced == 0 && radix_left == 0 && ntiles > BUCKET_LOCAL_TILES && last_I > BUCKET_LOCAL_AVG * ntiles && last_I <= LOCAL_AVG * ntiles;
}

// The fifth binning plan, "cells": the fourth plan's emission, key and finish by the compositing kernel, but the instances are partitioned
// without a chain — one pass by the top eight partition bits into ranges reserved on per-bin cursors, then every cell ordered by the low
// eight through LDS, tile ranges included (cell_sort.hip).  Its passes are not stable; local_order_tile breaks ties by Gaussian id, so the
// lists come out the same bits.  Holds where bucket_local_rule holds and the partition key is 8 or 16 bits wide (one or two tile passes:
// up to 2^14 tiles; a 24-bit key would leave the finish 2^16 bins per cell); the compositing kernel and the back-off (too_long, radix_left,
// clean) are the fourth plan's.  by_shape: CELLS_BY_SHAPE — whether the shapes bucket_local_rule picks take it unforced (ledger (cr)).
// forced: DAS3R_BINNING=cells (5); where the rule does not hold it falls where DAS3R_BINNING=bucket falls.
constexpr bool CELLS_BY_SHAPE = true;
static inline bool cells_rule(int forced, bool bucket_local, int tile_passes, bool by_shape = CELLS_BY_SHAPE) {
    return bucket_local && tile_passes <= 2 && (forced == 5 || (forced == 0 && by_shape));
}

// What the last forward of the current shape (P, W, H) taught us.
struct Verdict {
    int P = 0, W = 0, H = 0;
    int64_t last_I = -1;             // the last forward's instance count; < 0: the shape has had no forward yet
    int64_t peak_I = 0;              // the largest count, slowly forgotten (learn_count)
    int radix_left = 0;              // forwards this shape still spends on the global sort
    int backoff = BACKOFF_MIN;       // ... and how many the next failure costs
    uint32_t gen = 0;                // the generation the kernels' mailbox words name (plan_forward)
    int seg_extra = 0;               // 1: the segmented path takes one more partition pass of bucket bits
    bool last_seg = false;           // the last forward was planned on the segmented path
    bool fine = false;               // skewed or crowded tile lists: the 2x2-region compositing kernels (learn_skew)
    uint32_t forwards = 0;           // forwards of the shape so far: the position in the re-decision schedule of `fine`
    uint32_t clean = 0;              // forwards planned on a fast path since the last failure
    uint32_t longest = 0;            // the longest tile list as last measured (backward_hint)
    static Verdict fresh(uint32_t gen) {
        Verdict v;
        v.gen = gen;
        return v;
    }
};

// das3r_raster_learning(set): the part of a Verdict a checkpoint carries, handed to the next shape the thread meets
struct Resume {
    bool valid = false, fine = false;
    uint32_t forwards = 0;
};

// Everything plan_forward / learn_count read that is not in the Verdict.
struct PolicyInputs {
    int P, W, H;
    int ntiles, tbits, tile_passes;   // Layout
    uint32_t too_long;     // mailbox word: != 0: a forward of the shape with that generation number met a list too long for LDS
    uint32_t want_bits;    // mailbox word: != 0: the segmented path of that generation sorted a segment long enough to want more bucket bits
    int forced;            // Switches::binning (DAS3R_BINNING=local | radix | seg | seg3 | bucket | cells: 1 | -1 | 2 | 3 | 4 | 5): force one (diagnostics, tests); 0: by shape
    bool onesweep;         // use_onesweep(): false only with the classic radix passes of an experiments build, which have no fast path
    int64_t capacity_hint; // das3r_raster_args: -1 = the caller wants the exact size
    bool capacity_exact;   // Switches::capacity_exact (DAS3R_CAPACITY=exact)
    Resume *resume;        // in/out: consumed by the first forward of a new shape (may be null)
};

struct ForwardPlan {
    bool local, seg;            // local order / segmented path; neither: the global depth sort
    bool bucket_local;          // (with seg) segmented emission and passes, no segment sort: the compositing kernel finishes the lists (bucket_local_rule)
    bool cells;                 // (with bucket_local) partitioned by reserved ranges and finished per cell instead of by the stable passes (cells_rule)
    int seg_bits, seg_passes;   // depth-bucket bits and partition passes the segmented path would take (applied to the layout when seg)
    bool speculate;             // enqueue the whole forward for `cap` instances before its own count is known
    int64_t cap;                // (with speculate)
    bool decide_fine;           // this forward looks at its tile lists (learn_skew)
    uint32_t gen;               // what this forward's kernels write into the mailbox words they raise
};

// Called once per forward, after the mailbox words were read and cleared and before anything is launched.
//
// Depth order: scenes with short tile lists (the 100 k-splat 1080p benchmark averages 32 entries per tile) skip the global
// depth sort — five of the eleven binning launches, each latency-bound at that size; the instances are emitted in index
// order and the compositing kernel sorts every tile's list itself (common.h: LocalBin).  Chosen from the instance count
// of the previous forward of the same shape, confirmed with this forward's count (learn_count); a list that outgrows LDS is
// still sorted correctly (slowly) and sends the next forwards back to the global sort.
static inline ForwardPlan plan_forward(Verdict &v, const PolicyInputs &in) {
    if (v.P != in.P || v.W != in.W || v.H != in.H) {
        v = Verdict::fresh(next_gen(v.gen));
        v.P = in.P;
        v.W = in.W;
        v.H = in.H;
        if (in.resume && in.resume->valid) {   // a resumed job: the forward-kernel choice and its schedule continue where the checkpoint left them
            v.fine = in.resume->fine;
            v.forwards = in.resume->forwards;
            in.resume->valid = false;
        }
    }
    ForwardPlan p;
    // Skewed tile lists -> the forward kernel with four workgroups per tile (render_regions.hip; learn_skew): decided from the
    // tile ranges of the shape's FIRST forward and of every 512th after it — a one-workgroup kernel behind the binning leaves the longest
    // list in the mailbox and the host waits for it (the first forward of a shape waits for its count anyway; afterwards one short wait
    // per 512 forwards).  Which kernel runs in which forward thus depends on the data alone, never on timing: the two kernels round a
    // pixel's T differently in the last bit, and a job must end bit-identical however it was scheduled.
    p.decide_fine = (v.forwards++ & (FINE_PERIOD - 1u)) == 0u;
    // Every decision below starts a new GENERATION of the shape: the words the kernels raise (too_long / want_bits) name the generation they were
    // launched under, and the host runs one or two forwards ahead of the device — the forward enqueued BEFORE a decision was taken raises
    // the same word again a moment later, and answered a second time it turned "one more partition pass" straight into "global sort for
    // 64 forwards" (round 6: seen as a smooth-depth train step of 1.29 ms instead of 1.18 on some boxes, its first 64 timed steps on the
    // global sort; which box depended on how far ahead its host ran).
    if (v.last_I < 0) {   // (a shape's first forward: nothing to learn from yet)
    } else if (in.too_long == v.gen && !(v.last_seg && v.seg_extra == 0 && in.tile_passes < 3 && seg_dbits(in.tbits, in.tile_passes + 1) > 0)) {
        // global sort for a while; longer every time it happens AGAIN SOON.  Round 6: a failure that comes after 256 or more clean forwards
        // on the fast path is an occasional one — a view of 45 that looks at a wall head-on (DAVIS-shaped job: one forward in ~ 350) — and
        // starts from the shortest stint again: the doubling never forgot, and by iteration 4000 such a job had spent 2 447 of its
        // iterations on the global sort (binning 0.64 ms against 0.47), tools/probes/job_binning_paths.py
        if (v.clean >= CLEAN_RESET) v.backoff = BACKOFF_MIN;
        v.radix_left = v.backoff;
        if (v.backoff < BACKOFF_MAX) v.backoff *= 2;
        v.clean = 0;
        v.gen = next_gen(v.gen);
    } else if (in.too_long == v.gen || in.want_bits == v.gen) {
        v.seg_extra = 1;                  // the segmented path with one more partition pass of bucket bits from now on (this shape);
                                          // a segment that is too long even then sends the shape back to the global sort (above)
        v.gen = next_gen(v.gen);
    }
    const int forced = in.forced;
    p.bucket_local = bucket_local_rule(forced, in.onesweep, in.tbits, in.tile_passes, in.ntiles, v.last_I, v.radix_left);
    // (DAS3R_BINNING=bucket where the key has no room for buckets: the local order)
    p.cells = cells_rule(forced, p.bucket_local, in.tile_passes);
    p.local = !p.bucket_local && in.onesweep && (forced == 1 || forced == 4 || forced == 5 || (forced == 0 && v.radix_left == 0 && v.last_I <= LOCAL_AVG * in.ntiles));
    // Long lists (round 4): the segmented path — no global depth sort; the tile partition's passes carry a depth bucket in the key bits
    // the tile ids leave free, and every (tile, bucket) segment is sorted inside LDS (segkey.h, segsort.hip).  Needs free key bits
    // and segments that stay short on average; a segment that did not fit in LDS sends the shape back to the global sort for a
    // while, like a list too long for the local order does (the same mailbox word and back-off).
    // The buckets are global: they split a tile's list well when its depths are spread (random-depth benchmarks) and badly when a tile
    // sees a thin depth band of a wide scene (every real scene: its Gaussians lie on surfaces).  A forward that had to rank a long
    // segment says so (want_bits), and the shape takes ONE MORE partition pass from then on: eight more bucket bits — a band
    // that held 3 % of the scene's instances in 4 of 128 buckets is cut into a thousand (r4, coherent-depth 5 M-splat scene:
    // segment sort 1.08 ms with two passes, see DESIGN.md with three).
    p.seg_passes = in.tile_passes + ((!p.bucket_local && (forced == 3 || (forced == 0 && v.seg_extra))) ? 1 : 0);
    p.seg_bits = (in.onesweep && p.seg_passes <= 3) ? seg_dbits(in.tbits, p.seg_passes) : 0;
    p.seg = p.bucket_local || (!p.local && p.seg_bits > 0 && (forced == 2 || forced == 3 || (forced == 0 && v.radix_left == 0 && v.last_I >= 0 &&
                                                                                              (v.last_I >> std::min(p.seg_bits, 20)) <= SEG_AVG * in.ntiles)));
    v.last_seg = p.seg && !p.bucket_local;   // (a list that outgrows LDS under the bucket-ordered local finish backs off as the local order does: no extra pass)
    if (p.local || p.seg) v.clean++;   // (a failure of this forward is reported to the next one: reset there)
    if (forced == 0 && v.radix_left > 0) v.radix_left--;
    // Local order or segments + a previous forward of the same shape: nothing else could be enqueued while the count is on its way, so
    // the binning buffer is laid out for that forward's count + 25 % and the whole forward is enqueued before the host looks
    // at the mailbox (the kernels clamp to the capacity).  Should the scene have grown past it, the binning and the
    // compositing are redone with the exact size.  DAS3R_CAPACITY=exact switches the speculation off.
    p.speculate = (p.local || p.seg) && v.last_I >= 0 && in.capacity_hint != -1 && !in.capacity_exact;   // (round 4: the segmented path too)
    // headroom: 25 % over the last count, 5 % over the (slowly forgotten) largest one — a camera that moves between views
    // of different density overflows rarely
    p.cap = p.speculate ? std::min(std::max(v.last_I + v.last_I / 4, v.peak_I + v.peak_I / 20) + 4096, CAPACITY_MAX) : 0;
    p.gen = v.gen;
    return p;
}

// This forward's count has arrived.  Returns whether a forward that planned the local order WITHOUT speculating must take the global
// sort after all (the scene grew; a speculative forward is enqueued by now and keeps its path).
static inline bool learn_count(Verdict &v, int64_t I, const PolicyInputs &in, const ForwardPlan &p) {
    v.last_I = I;
    v.peak_I = std::max(I, v.peak_I - v.peak_I / 1024);
    return p.local && in.forced == 0 && I > LOCAL_AVG * in.ntiles;
}

// The mean list length learn_skew measures the longest against: the last count the shape has learnt (a speculative forward looks at its
// lists before its own count is stored: the previous forward's; an exact one after: its own), the capacity on a shape's first.
static inline int64_t skew_mean(const Verdict &v, int64_t cap, int ntiles) { return (v.last_I > 0 ? v.last_I : cap) / std::max(ntiles, 1); }

// A forward with ForwardPlan::decide_fine has measured its tile lists (render_regions.hip list_skew_kernel): the longest, and of 64
// consecutive list entries those in the tile's fullest quadrant, x 16.  Returns Verdict::fine.
// skewed: 1.8 x the mean list, the measured crossover of the forward kernels (ledger (bd)); crowded: a stretch of a list sits in part of
// its tile (random depths: 20 of 64 in the fullest quadrant) — there the 2x2-region kernels win both ways whatever the skew (ledger (be))
static inline bool learn_skew(Verdict &v, uint32_t longest32, uint32_t crowd16, int64_t cap, int ntiles) {
    const int64_t longest = (int64_t)longest32, mean = skew_mean(v, cap, ntiles);
    v.longest = longest32;   // (what the backward's grid is sized by until the next look: backward_hint)
    v.fine = (longest > mean + (mean * 4) / 5 && longest >= 4096) || crowd16 >= CROWDED16;
    return v.fine;
}

// das3r_raster_saved.flags of a forward composited with the 2x2-region kernels, for the backward pass of that forward (kernel_choice.h choose_backward):
// bit 0, and in bits 8 - 15 the buckets (`bucket` list positions each: common.h BUCKET) of the shape's longest tile list as last
// measured, + 2 of headroom — the bucket-parallel backward launches that many workgroups per tile instead of the AVERAGE list's (a tile
// of four times the mean then takes four buckets per workgroup, back to back, and the kernel ends with them: self-consistent job
// 0.409 -> 0.313 ms)
static inline uint32_t backward_hint(const Verdict &v, uint32_t bucket) { return 1u | (std::min<uint32_t>(63u, v.longest / bucket + 2u) << 8); }

static inline bool prefers_regions(const Verdict &v) { return v.fine; }
static inline uint32_t forwards_seen(const Verdict &v) { return v.forwards; }

// das3r_raster_forget_shapes.  (Generation numbers keep counting: a word a forward of the old shape still has on its way names nobody.)
static inline void forget(Verdict &v) { v = Verdict::fresh(v.gen); }

// das3r_raster_learning(set): forget the shapes and hand (fine, forwards) to the next shape plan_forward meets — that one only, once.
static inline void resume(Verdict &v, Resume &r, bool fine, uint32_t forwards) {
    forget(v);
    r.valid = true;
    r.fine = fine;
    r.forwards = forwards;
}

// A Verdict and its Resume as a plain struct of integers with the same field names (das3r_path_policy_state, include/das3r_raster.h)
template <class S>
static inline void policy_state_from(const S &s, Verdict *v, Resume *r) {
    v->P = s.P, v->W = s.W, v->H = s.H;
    v->last_I = s.last_I, v->peak_I = s.peak_I;
    v->radix_left = s.radix_left, v->backoff = s.backoff;
    v->gen = s.gen;
    v->seg_extra = s.seg_extra;
    v->last_seg = s.last_seg != 0, v->fine = s.fine != 0;
    v->forwards = s.forwards, v->clean = s.clean, v->longest = s.longest;
    r->valid = s.resume_valid != 0, r->fine = s.resume_fine != 0, r->forwards = s.resume_forwards;
}
template <class S>
static inline void policy_state_to(const Verdict &v, const Resume &r, S *s) {
    s->P = v.P, s->W = v.W, s->H = v.H;
    s->last_I = v.last_I, s->peak_I = v.peak_I;
    s->radix_left = v.radix_left, s->backoff = v.backoff;
    s->gen = v.gen;
    s->seg_extra = v.seg_extra;
    s->last_seg = v.last_seg, s->fine = v.fine;
    s->forwards = v.forwards, s->clean = v.clean, s->longest = v.longest;
    s->resume_valid = r.valid, s->resume_fine = r.fine, s->resume_forwards = r.forwards;
}

}  // namespace das3r
