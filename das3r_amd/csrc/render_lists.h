// render_lists.h — the walk over the tile lists a forward has left behind, as the kernels of render_aux.hip, render_aux_bwd.hip and
// render_distort.hip share it.  A kernel on these lists is a per-pair body and a payload; everything else is here.
//
// Decomposition (render_common.h's): one 256-lane workgroup per 16x16 tile, one wave64 per 8x8 quadrant, the list staged through LDS in
// batches of 256 entries — (xy, conic + opacity[, emission slot][, the kernel's payload]) — front to back or reversed, every wave culling a
// batch against its quadrant with four ballots and walking the bits that are left.  A pixel takes part in list position k iff
// k < n_contrib[pixel] — the forward's own stop, not a re-derived T < 1e-4 — and alpha is pair_alpha's, the expression and the two tests of
// every compositing kernel.  The early-outs are the walk's, not a body's: a wave leaves a front-to-back batch at the first position at or
// past its pixels' last stop (wmax), skips such positions back to front, and skips a pair no lane of which is active.
//
// Back to front the per-pair values are reduced over the wave's 64 pixels on the cross-lane network, every wave STORING its totals into
// its own LDS column (WaveColumns: a (wave, entry) pair is visited at most once per batch) and remembering which entries it stored in a
// 128-bit mask; the four columns are added in the order 0, 1, 2, 3, a column that was not stored counting as 0 (a select: what the LDS held
// before does not matter, and no column needs zeroing), the moments become replay_pair's sums (moments_to_sums) and the nine-float row goes
// to the entry's emission slot.  The 256 staged entries are walked and flushed in two halves of 128, which halves the columns.  No
// floating-point atomics, no unordered LDS adds: bit-identical from run to run.  Rows of list entries no pixel reaches are zeroed
// (zero_unreached_rows): nothing needs pre-zeroing.
#pragma once
#include "render_common.h"

namespace das3r {

// What every kernel on a forward's saved lists reads (by value: a kernel argument).
struct ListArgs {
    const uint2 *ranges;
    const uint32_t *point_list;
    int W, H, tiles_x, packed_tiles /*render_common.h pack_tiles*/;
    const float4 *xyh, *conic_opacity, *rgbd;
    const uint32_t *n_contrib;
    const float *final_T;
    const uint32_t *slot_list;   // emission slot of every list entry = its row of the per-instance arrays
    uint32_t last_g, cap;
};

static inline ListArgs list_args(const Buffers &v, int W, int H, int P) {
    return {v.ranges(), v.point_list(), W, H, v.L.tiles_x, pack_tiles(v.L),
            v.xy(), v.conic_opacity(), v.rgbd(),
            v.n_contrib(), v.final_T(), v.b_slot(),
            (uint32_t)(P - 1), (uint32_t)v.L.capacity};
}

// lanes of a wave: the largest value among them (uniform)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// One lane's view of its tile: lane `lane` of the wave is a pixel of the 8x8 quadrant `quad`.
struct TileLane {
    int tile;   // < 0: the block has no tile (the whole workgroup leaves)
    int bx, by, px, py;
    bool inside;
    float pxf, pyf, qcx, qcy;   // the pixel, the quadrant's centre
    uint2 range;
    uint32_t len;
    size_t pix;
    uint32_t last_contributor;   // n_contrib of the pixel (0 outside the image)
    uint32_t wmax;               // no pixel of this wave blended anything at or past this list position (in a scalar register)
    uint32_t wmax_lanes;         // the same value as the reduction left it, one copy per lane (the split aux forward's loop: render_aux.hip)
    uint32_t max_contrib;        // no pixel of the tile did at or past this one (<= len)
};

// tile_block: the block's place in xcd_grid's order; quad: the quadrant this wave's lanes are the pixels of (a kernel with one workgroup per
// tile: the wave's number).  Holds a barrier: every wave of the workgroup calls it.
__device__ __forceinline__ TileLane tile_lane(const ListArgs &a, const int tile_block, const int quad) {
    __shared__ uint32_t s_max[4];
    TileLane t;
    t.tile = xcd_tile(tile_block, a.packed_tiles, a.tiles_x);
    if (t.tile < 0) return t;
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    t.bx = t.tile % a.tiles_x, t.by = t.tile / a.tiles_x;
    quadrant_pixel(t.bx, t.by, quad, lane, t.px, t.py);
    t.inside = t.px < a.W && t.py < a.H;
    t.pxf = (float)t.px, t.pyf = (float)t.py;
    t.qcx = (float)(t.bx * TILE_X + ((quad & 1) << 3)) + 3.5f, t.qcy = (float)(t.by * TILE_Y + ((quad >> 1) << 3)) + 3.5f;
    t.range = safe_range(a.ranges[t.tile], a.cap);
    t.len = t.range.y - t.range.x;
    t.pix = (size_t)t.py * a.W + t.px;
    t.last_contributor = t.inside ? a.n_contrib[t.pix] : 0u;
    t.wmax_lanes = wave_max_u32(t.last_contributor);
    t.wmax = __builtin_amdgcn_readfirstlane(t.wmax_lanes);   // (uniform already: in a scalar register the walk's tests on it are branches)
    if (lane == 0) s_max[wave] = t.wmax;
    __syncthreads();
    t.max_contrib = min(max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])), t.len);
    return t;
}

// Stages n <= 256 list entries: staged entry j holds list index first + j (REVERSED: first - j).  s_slot: null where the kernel writes no
// per-instance row.  payload(j, g): the kernel's own columns of staged entry j, Gaussian g.
struct NoPayload {
    __device__ __forceinline__ void operator()(int, uint32_t) const {}
};
template <bool REVERSED, class Payload>
__device__ __forceinline__ void stage_batch(const ListArgs &a, const uint32_t first, const int n, float4 *s_xyh, float4 *s_co, uint32_t *s_slot,
                                            Payload payload) {
    const int tid = threadIdx.x;
    if (tid < n) {
        const uint32_t pos = REVERSED ? first - (uint32_t)tid : first + (uint32_t)tid;
        const uint32_t g = min(a.point_list[pos], a.last_g);
        if (s_slot != nullptr) s_slot[tid] = min(a.slot_list[pos], a.cap - 1u);
        s_xyh[tid] = a.xyh[(size_t)g * SPLAT_REC];
        s_co[tid] = a.conic_opacity[(size_t)g * SPLAT_REC];
        payload(tid, g);
    }
}

// the staged entries that reach this wave's quadrant, 64 per mask (wave_in false: none — uniform)
__device__ __forceinline__ void cull_batch(const TileLane &t, const float4 *s_xyh, const int n, const bool wave_in, uint64_t masks[4]) {
    const int lane = __lane_id();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int s = k * 64 + lane;
        masks[k] = wave_in ? __ballot(s < n && quadrant_hit(s_xyh[s], t.qcx, t.qcy)) : 0ull;
    }
}

// One staged batch front to back (staged entry 0 is list position first): body(j, position, active, alpha, G, dx, dy) for every pair some
// lane of the wave blends.  Holds no barrier.
template <class Body>
__device__ __forceinline__ void walk_front_to_back(const TileLane &t, const float4 *s_xyh, const float4 *s_co, const int n, const uint32_t first,
                                                   Body body) {
    if (first >= t.wmax) return;   // (wave-uniform)
    uint64_t masks[4];
    cull_batch(t, s_xyh, n, true, masks);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint64_t m = masks[k];
        while (m != 0ull) {
            const int j = k * 64 + __builtin_ctzll(m);
            m &= m - 1ull;
            const uint32_t position = first + (uint32_t)j;   // 0-based list position
            if (position >= t.wmax) break;                   // (uniform: the bits come in list order)
            const float4 p = s_xyh[j];
            const float4 co = s_co[j];
            float dx, dy, G, alpha;
            const bool active = pair_alpha(p.x, p.y, co, t.pxf, t.pyf, dx, dy, G, alpha) & (position < t.last_contributor);
            if (__ballot(active) == 0ull) continue;
            body(j, position, active, alpha, G, dx, dy);
        }
    }
}

// A tile's list front to back, one workgroup per tile: the positions some pixel reaches, in batches of 256.
template <class Payload, class Body>
__device__ __forceinline__ void walk_list_front_to_back(const ListArgs &a, const TileLane &t, float4 *s_xyh, float4 *s_co, Payload payload, Body body) {
    const int rounds = ((int)t.max_contrib + TILE_PIX - 1) / TILE_PIX;
    for (int i = 0; i < rounds; i++) {
        const int done_before = i * TILE_PIX;
        const int n = min(TILE_PIX, (int)t.max_contrib - done_before);
        if (i > 0) __syncthreads();   // the previous batch has been read by every wave
        stage_batch<false>(a, t.range.x + (uint32_t)done_before, n, s_xyh, s_co, nullptr, payload);
        __syncthreads();
        walk_front_to_back(t, s_xyh, s_co, n, (uint32_t)done_before, body);   // (the barriers above are taken by every wave)
    }
}

// rows[slot of list index first + t][0 .. NCOLS) = 0 for t < count: the rows of list entries no pixel reaches (cap > 0 whenever a list has
// entries)
template <int NCOLS>
__device__ __forceinline__ void zero_unreached_rows(const ListArgs &a, float *rows, const uint32_t first, const uint32_t count) {
    const uint32_t ntail = count * NCOLS;
    for (uint32_t f = threadIdx.x; f < ntail; f += TILE_PIX) {
        const uint32_t e = f / NCOLS, q = f - e * NCOLS;
        rows[(size_t)min(a.slot_list[first + e], a.cap - 1u) * NCOLS + q] = 0.f;
    }
}

// ---- back to front: the replay of the two geometry backward kernels ----
constexpr int LIST_HALF = TILE_PIX / 2;   // the staged batch is walked and flushed in two halves: half the column storage
static_assert((LIST_HALF & (LIST_HALF - 1)) == 0 && LIST_HALF % 64 == 0, "an entry's place in its half is j & (LIST_HALF - 1); a half is whole masks");

// NV values per (wave, entry): the six moments of replay_pair_moments first, then the kernel's own
template <int NV>
struct WaveColumns {
    float col[4][LIST_HALF * NV];         // col[wave][jl * NV + q]: the wave's total of value q for entry jl of the half, where it stored one
    unsigned long long vis[4][2];    // vis[wave][kk] bit b: the wave stored its totals for entry 64 kk + b of the half
};

// eight per-lane values of staged entry j -> their wave totals -> values first .. first + 7 (those below NV) of the wave's column: a plain
// store, (wave, entry) pairs are visited once
template <int NV>
__device__ __forceinline__ void store_totals8(WaveColumns<NV> &wc, const int j, const float v8[8], const int first) {
    const int lane = __lane_id();
    const float r = wave_reduce8_transposed(v8, lane);   // lane l holds the total of value l >> 3
    if ((lane & 7) == 0 && first + (lane >> 3) < NV) wc.col[threadIdx.x >> 6][(j & (LIST_HALF - 1)) * NV + first + (lane >> 3)] = r;
}

// value q of entry jl of the half: the four waves' totals in a fixed order
template <int NV>
__device__ __forceinline__ float sum_columns(const WaveColumns<NV> &wc, const int jl, const int q) {
    const int kk = jl >> 6, b = jl & 63, f = jl * NV + q;
    const bool have0 = (wc.vis[0][kk] >> b) & 1ull, have1 = (wc.vis[1][kk] >> b) & 1ull, have2 = (wc.vis[2][kk] >> b) & 1ull,
               have3 = (wc.vis[3][kk] >> b) & 1ull;
    return (((have0 ? wc.col[0][f] : 0.f) + (have1 ? wc.col[1][f] : 0.f)) + (have2 ? wc.col[2][f] : 0.f)) + (have3 ? wc.col[3][f] : 0.f);
}

// The nh entries of half h -> the rows of their emission slots: partial [capacity, 9] = (value 6 if COL0, else 0; 0; 0; replay_pair's six
// geometry sums), and with NF > 0 partial_f [capacity, NF] = values 6 .. 6 + NF - 1.
template <int NV, bool COL0, int NF>
__device__ __forceinline__ void flush_half(const ListArgs &a, const WaveColumns<NV> &wc, const float4 *s_co, const uint32_t *s_slot, const int h,
                                           const int nh, float *partial, float *partial_f) {
    const int tid = threadIdx.x;
    if (tid < nh) {
        const int j = h * LIST_HALF + tid;
        float row[9];
        row[0] = COL0 ? sum_columns(wc, tid, 6) : 0.f;
        row[1] = 0.f;
        row[2] = 0.f;
#pragma unroll
        for (int q = 0; q < 6; q++) row[3 + q] = sum_columns(wc, tid, q);
        moments_to_sums(row, s_co[j], 0.5f * a.W, 0.5f * a.H);   // once per (tile, splat)
        float *out = partial + (size_t)s_slot[j] * 9;
#pragma unroll
        for (int q = 0; q < 9; q++) out[q] = row[q];
    }
    if constexpr (NF > 0) {
        for (int f = tid; f < nh * NF; f += TILE_PIX) {
            const int jl = f / NF, q = f - jl * NF;
            partial_f[(size_t)s_slot[h * LIST_HALF + jl] * NF + q] = sum_columns(wc, jl, 6 + q);
        }
    }
}

// A tile's list back to front, one workgroup per tile: every row of `partial` (and with NF > 0 of partial_f) that belongs to a list entry of
// the tile is written.  body(j, position, active, alpha, G, dx, dy) runs the pixel's recurrence and stores the pair's totals (store_totals8).
template <int NV, bool COL0, int NF, class Payload, class Body>
__device__ __forceinline__ void walk_list_back_to_front(const ListArgs &a, const TileLane &t, float4 *s_xyh, float4 *s_co, uint32_t *s_slot,
                                                        WaveColumns<NV> &wc, float *partial, float *partial_f, Payload payload, Body body) {
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    zero_unreached_rows<9>(a, partial, t.range.x + t.max_contrib, t.len - t.max_contrib);
    if constexpr (NF > 0) zero_unreached_rows<NF>(a, partial_f, t.range.x + t.max_contrib, t.len - t.max_contrib);

    const int rounds = ((int)t.max_contrib + TILE_PIX - 1) / TILE_PIX;
    for (int i = 0; i < rounds; i++) {
        const int done_before = i * TILE_PIX;
        const int n = min(TILE_PIX, (int)t.max_contrib - done_before);
        // the batch in reverse list order: staged entry j holds list position last - j
        const uint32_t last = t.max_contrib - 1u - (uint32_t)done_before;
        stage_batch<true>(a, t.range.x + last, n, s_xyh, s_co, s_slot, payload);
        __syncthreads();

        // the batch's positions are last + 1 - n .. last: all at or past this wave's last one?
        const bool wave_in = t.max_contrib - (uint32_t)done_before - (uint32_t)n < t.wmax;   // (wave-uniform; the barriers are taken by every wave)
        uint64_t masks[4];
        cull_batch(t, s_xyh, n, wave_in, masks);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (h * LIST_HALF >= n) continue;   // (uniform over the workgroup: n is)
            const int nh = min(LIST_HALF, n - h * LIST_HALF);
            unsigned long long vis[2] = {0ull, 0ull};   // (wave-uniform)
#pragma unroll
            for (int kk = 0; kk < 2; kk++) {
                uint64_t m = masks[2 * h + kk];
                while (m != 0ull) {
                    const int b = __builtin_ctzll(m), j = h * LIST_HALF + kk * 64 + b;
                    m &= m - 1ull;
                    const uint32_t position = last - (uint32_t)j;   // 0-based list position, descending
                    if (position >= t.wmax) continue;               // (uniform)
                    const float4 p = s_xyh[j];
                    const float4 co = s_co[j];
                    float dx, dy, G, alpha;
                    const bool active = pair_alpha(p.x, p.y, co, t.pxf, t.pyf, dx, dy, G, alpha) & (position < t.last_contributor);
                    if (__ballot(active) == 0ull) continue;   // (uniform) nobody's state changes: the entry's column stays unstored = 0
                    body(j, position, active, alpha, G, dx, dy);
                    vis[kk] |= 1ull << b;
                }
            }
            if (lane < 2) wc.vis[wave][lane] = lane == 0 ? vis[0] : vis[1];
            __syncthreads();
            flush_half<NV, COL0, NF>(a, wc, s_co, s_slot, h, nh, partial, partial_f);
            __syncthreads();   // before the columns are stored again, and before the next batch is staged over this one
        }
    }
}

}  // namespace das3r
