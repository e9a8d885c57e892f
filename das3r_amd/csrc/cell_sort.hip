// cell_sort.hip — the fifth binning plan, "cells" (path_policy.h cells_rule): the bucket plan's emission and key
// (tile << (dbits + fbits) | bucket << fbits | fraction: segkey.h), partitioned WITHOUT a chain.  The one-sweep passes
// (sort_onesweep.hip) are stable, which costs them a look-back over the counts of every earlier workgroup; the compositing
// kernel that finishes the lists (render_common.h local_order_tile) ranks every entry itself and breaks ties by Gaussian id,
// so the order in which the entries of a (tile, bucket) segment arrive means nothing — and then no workgroup needs another's
// counts, only a place of its own inside a bin:
//   A  cell_partition_kernel  one pass over the emitted (key, id, slot) triples by the TOP eight partition bits (a "cell": the
//      tiles that share them).  The bin bases are known up front — scan_emit_kernel leaves the histogram of every digit in
//      ghist before any pass starts — and a workgroup reserves its run inside a bin with one returning atomic add per non-empty
//      digit on that bin's cursor (256 words, a 128-byte line each on large scenes, zeroed with ghist by the same forward).
//   B  cell_finish_kernel     every cell's run is ordered by the LOW eight partition bits (tile in cell, bucket) through LDS and
//      written out unit-stride, with the tile ranges of the cell and the forward's self-check word: no tile_ranges launch.
// Neither kernel waits for another workgroup: no ticket, no status rows, no polling; every loop is bounded by a count read once.
// With eight partition bits in all (at most 64 tiles) there is one cell and B alone runs, on the emitted triples.
// CPU model: tests/test_cell_sort_model.py.
#include "granule.h"

namespace das3r {

#ifndef DAS3R_CELL_SPLIT
#define DAS3R_CELL_SPLIT 4      // workgroups per cell, each finishing 256 / SPLIT consecutive bins
#endif
#ifndef DAS3R_CELL_ROUND
#define DAS3R_CELL_ROUND 3072   // entries of an LDS round of B: 36 KB of staging, four workgroups per CU
#endif
#ifndef DAS3R_CELL_B1
#define DAS3R_CELL_B1 8        // keys a thread has in flight per trip of phase 1
#endif
#ifndef DAS3R_CELL_B2
#define DAS3R_CELL_B2 4        // triples a thread has in flight per trip of phase 2
#endif
constexpr int CELL_SPLIT = DAS3R_CELL_SPLIT, CELL_ROUND = DAS3R_CELL_ROUND;
static_assert(CELL_SPLIT >= 1 && CELL_SPLIT <= 8 && (CELL_SPLIT & (CELL_SPLIT - 1)) == 0, "a power of two of workgroups per cell");

// A.  Ranking and staging as in onesweep_pass_kernel (wave-private counters, match-any); what replaces the look-back is the
// reservation.  The first pass of the plan: the slot payload is the input index.
template <int IPL>
__global__ void __launch_bounds__(256) cell_partition_kernel(const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ gid_in,
                                                             uint32_t *__restrict__ keys_out, uint32_t *__restrict__ gid_out,
                                                             uint32_t *__restrict__ slot_out, uint32_t cap, const uint32_t *__restrict__ n_ptr,
                                                             int shift, const uint32_t *__restrict__ ghist /*[256] this digit*/,
                                                             uint32_t *__restrict__ cursor /*[256 * cursor_stride], zero*/, int cursor_stride,
                                                             uint32_t *__restrict__ err) {
    __shared__ uint16_t cnt[4][RADIX_SIZE];   // per-wave digit counts, then per-wave running offsets
    __shared__ uint32_t gdelta[RADIX_SIZE];
    __shared__ uint32_t sk[256 * IPL], sv[256 * IPL], sv2[256 * IPL];
    __shared__ uint32_t ws[8];
    const int tid = threadIdx.x, lane = __lane_id(), wave = tid >> 6;
    const uint32_t n = min(*n_ptr, cap);
    const uint32_t b = blockIdx.x;
    if ((uint64_t)b * 256u * IPL >= n) return;   // (the grid is sized for the capacity)
#pragma unroll
    for (int w = 0; w < 4; w++) cnt[w][tid] = 0;
    __syncthreads();
    const uint32_t base = (b * 4u + (uint32_t)wave) * 64u * (uint32_t)IPL;

    uint32_t k[IPL], v[IPL];
#pragma unroll
    for (int s = 0; s < IPL; s++) {
        const uint32_t i = base + s * 64 + lane;
        k[s] = i < n ? keys_in[i] : 0u;
        v[s] = i < n ? gid_in[i] : 0u;
    }
    uint32_t local[IPL];
    {
        volatile uint16_t *cw = cnt[wave];
#pragma unroll
        for (int s = 0; s < IPL; s++) {
            const uint32_t i = base + s * 64 + lane;
            const bool valid = i < n;
            const uint32_t digit = (k[s] >> shift) & 255u;
            const uint64_t vm = __ballot(valid);
            uint32_t plo = (uint32_t)vm, phi = (uint32_t)(vm >> 32);
#pragma unroll
            for (int bb = 0; bb < RADIX_BITS; bb++) {
                const uint32_t sel = 0u - ((digit >> bb) & 1u);
                const uint64_t m = __ballot((digit >> bb) & 1u);
                plo &= ~((uint32_t)m ^ sel);
                phi &= ~((uint32_t)(m >> 32) ^ sel);
            }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
            const uint32_t count = (uint32_t)__popc(plo) + (uint32_t)__popc(phi);
            uint32_t before = 0;
            if (valid) before = cw[digit];
            __builtin_amdgcn_wave_barrier();
            if (valid && rank == 0) cw[digit] = (uint16_t)(before + count);
            __builtin_amdgcn_wave_barrier();
            local[s] = before + rank;
        }
    }
    __syncthreads();

    // thread d owns digit d: reserve this workgroup's run of the digit first (one trip to the cursor's line), stage while it is on its way
    const uint32_t c0 = cnt[0][tid], c1 = cnt[1][tid], c2 = cnt[2][tid], c3 = cnt[3][tid];
    const uint32_t total = c0 + c1 + c2 + c3;
    uint32_t reserved = 0u;
    if (total) reserved = __hip_atomic_fetch_add(cursor + (size_t)tid * cursor_stride, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t g = ghist[tid];
    uint32_t digit_base, lstart;
    {
        const uint32_t incl = wave_incl_scan_u32(g), lincl = wave_incl_scan_u32(total);
        if (lane == 63) {
            ws[wave] = incl;
            ws[4 + wave] = lincl;
        }
        __syncthreads();
        uint32_t wbase = 0, lbase = 0;
#pragma unroll
        for (int w = 0; w < 4; w++)
            if (w < wave) {
                wbase += ws[w];
                lbase += ws[4 + w];
            }
        lstart = lbase + lincl - total;
        digit_base = wbase + incl - g;
        cnt[0][tid] = (uint16_t)lstart;
        cnt[1][tid] = (uint16_t)(lstart + c0);
        cnt[2][tid] = (uint16_t)(lstart + c0 + c1);
        cnt[3][tid] = (uint16_t)(lstart + c0 + c1 + c2);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < IPL; s++) {
        const uint32_t i = base + s * 64 + lane;
        if (i < n) {
            const uint32_t slot = cnt[wave][(k[s] >> shift) & 255u] + local[s];
            sk[slot] = k[s];
            sv[slot] = v[s];
            sv2[slot] = i;
        }
    }
    if (reserved + total > g) atomicOr(err, ERR_COUNTS);   // self-check: a bin never holds more than the histogram says
    gdelta[tid] = digit_base + reserved - lstart;           // destination of staged slot i holding digit d: i + gdelta[d]
    __syncthreads();

    const uint32_t block_first = b * 256u * (uint32_t)IPL;
    const uint32_t nvalid = min(n - block_first, 256u * (uint32_t)IPL);
#pragma unroll
    for (int s = 0; s < IPL; s++) {
        const uint32_t i = s * 256 + tid;
        if (i < nvalid) {
            const uint32_t key = sk[i];
            const uint32_t dst = i + gdelta[(key >> shift) & 255u];
            if (dst >= n) {   // never write out of bounds, whatever went wrong upstream
                atomicOr(err, ERR_RANGE);
                continue;
            }
            keys_out[dst] = key;
            gid_out[dst] = sv[i];
            slot_out[dst] = sv2[i];
        }
    }
}

// B.  Workgroup (cell, part) of CELL_SPLIT: the cell's whole 256-bin histogram from its keys (phase 1: every part recomputes it, so
// the parts share nothing), then bins [part, part + 1) * 256 / CELL_SPLIT in rounds of contiguous bins that fit the staging area
// (phase 2: the cell's triples are streamed again, the round's entries take their place with an LDS atomic on their bin's counter and
// leave unit-stride).  A bin longer than a round is scattered to its place directly and reported in the too_long mailbox word: its
// tile's list is longer than anything the compositing kernel orders in LDS.  The parts of a cell are blockIdx.x, + 8, + 16, ...: one XCD.
__global__ void __launch_bounds__(256) cell_finish_kernel(const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ gid_in,
                                                          const uint32_t *__restrict__ slot_in /*null: the input index*/,
                                                          uint32_t *__restrict__ keys_out, uint32_t *__restrict__ gid_out,
                                                          uint32_t *__restrict__ slot_out, uint32_t cap, const uint32_t *__restrict__ n_ptr,
                                                          int kshift, int dbits, uint32_t ntiles, uint32_t ncells,
                                                          const uint32_t *__restrict__ ghist_hi /*[256] cell sizes; null: one cell*/,
                                                          const uint32_t *__restrict__ cursor /*A's, for the self-check; null: none*/, int cursor_stride,
                                                          uint2 *__restrict__ ranges, const uint32_t *__restrict__ err,
                                                          uint32_t *__restrict__ host_late, uint32_t tag, uint32_t inject,
                                                          uint32_t *__restrict__ host_flag, uint32_t flag_value) {
    __shared__ uint32_t s_off[RADIX_SIZE + 1], s_cur[RADIX_SIZE], ws[4], s_cell[2];
    __shared__ uint32_t st_k[CELL_ROUND], st_g[CELL_ROUND], st_s[CELL_ROUND];
    const int tid = threadIdx.x;
    const uint32_t n = min(*n_ptr, cap);
    if (blockIdx.x == 0) {   // last binning kernel: hand the self-check word of this forward to the host mailbox (mailbox.h)
        const bool bad = cursor && ghist_hi && cursor[(size_t)tid * cursor_stride] != ghist_hi[tid];   // every bin of A filled exactly
        const int any = __syncthreads_or(bad ? 1 : 0);
        if (tid == 0 && host_late) {
            host_late[0] = *err | inject | (any ? ERR_COUNTS : 0u);
            __hip_atomic_store(host_late + 1, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    const uint32_t cell = (blockIdx.x / (8u * CELL_SPLIT)) * 8u + (blockIdx.x & 7u), part = (blockIdx.x >> 3) & (CELL_SPLIT - 1u);
    if (cell >= ncells) return;
    {
        const uint32_t c = ghist_hi ? ghist_hi[tid] : (tid == 0 ? n : 0u);
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan_256(c, ws, &tot);
        if ((uint32_t)tid == cell) {
            s_cell[0] = min(ex, n);
            s_cell[1] = min(c, n - min(ex, n));
        }
        s_cur[tid] = 0u;   // phase 1's histogram
        __syncthreads();
    }
    const uint32_t base = s_cell[0], cnt = s_cell[1];
    if (cnt == 0u) return;   // (uniform) an empty cell: its tiles keep the empty ranges the preprocess kernel left
    const uint32_t *kin = keys_in + base;

    constexpr int B1 = DAS3R_CELL_B1;
    for (uint32_t i0 = 0; i0 < cnt; i0 += 256u * B1) {
        uint32_t k[B1];
#pragma unroll
        for (int u = 0; u < B1; u++) {
            const uint32_t i = i0 + u * 256u + tid;
            k[u] = i < cnt ? kin[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < B1; u++)
            if (i0 + u * 256u + tid < cnt) atomicAdd(&s_cur[(k[u] >> kshift) & 255u], 1u);
    }
    __syncthreads();
    {
        const uint32_t h = s_cur[tid];
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan_256(h, ws, &tot);
        s_off[tid] = ex;
        if (tid == 255) s_off[256] = ex + h;
        __syncthreads();
    }
    if (part == 0u && tid < (1 << (8 - dbits))) {   // the ranges of the cell's tiles (an empty tile keeps its zeroes)
        const uint32_t t = (cell << (8 - dbits)) + (uint32_t)tid;
        const uint32_t lo = s_off[tid << dbits], hi = s_off[(tid + 1) << dbits];
        if (hi > lo && t < ntiles) ranges[t] = make_uint2(base + lo, base + hi);
    }

    constexpr int B2 = DAS3R_CELL_B2;
    const int b_end = (int)(part + 1u) * (RADIX_SIZE / CELL_SPLIT);
    int r0 = (int)part * (RADIX_SIZE / CELL_SPLIT);
    while (r0 < b_end) {   // (uniform: bounded by the bins)
        const uint32_t first = s_off[r0], lim = first + (uint32_t)CELL_ROUND;
        int lo = r0, hi = b_end;
        while (lo < hi) {   // the last bin boundary within a round of r0
            const int mid = (lo + hi + 1) >> 1;
            if (s_off[mid] <= lim) lo = mid;
            else hi = mid - 1;
        }
        const bool direct = lo == r0;   // bin r0 alone is longer than a round
        const int r1 = direct ? r0 + 1 : lo;
        const uint32_t m = s_off[r1] - first;
        if (m == 0u) {
            r0 = r1;
            continue;
        }
        __syncthreads();   // (the previous round's staging area has left; phase 1's histogram has been read)
        s_cur[tid] = 0u;
        __syncthreads();
        for (uint32_t i0 = 0; i0 < cnt; i0 += 256u * B2) {
            uint32_t k[B2], g[B2], sl[B2];
#pragma unroll
            for (int u = 0; u < B2; u++) {
                const uint32_t i = i0 + u * 256u + tid;
                const bool in = i < cnt;
                k[u] = in ? kin[i] : 0u;
                g[u] = in ? gid_in[base + i] : 0u;
                sl[u] = (in && slot_in) ? slot_in[base + i] : base + i;
            }
#pragma unroll
            for (int u = 0; u < B2; u++) {
                const int bin = (int)((k[u] >> kshift) & 255u);
                if (i0 + u * 256u + tid < cnt && bin >= r0 && bin < r1) {
                    const uint32_t at = s_off[bin] - first + atomicAdd(&s_cur[bin], 1u);
                    if (direct) {
                        const uint32_t dst = base + first + at;
                        if (at < m && dst < n) {
                            keys_out[dst] = k[u];
                            gid_out[dst] = g[u];
                            slot_out[dst] = sl[u];
                        }
                    } else if (at < (uint32_t)CELL_ROUND) {
                        st_k[at] = k[u];
                        st_g[at] = g[u];
                        st_s[at] = sl[u];
                    }
                }
            }
        }
        if (direct) {
            if (tid == 0 && host_flag) __hip_atomic_store(host_flag, flag_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else {
            __syncthreads();
            for (uint32_t j = tid; j < m; j += 256u) {
                const uint32_t dst = base + first + j;
                if (dst < n) {
                    keys_out[dst] = st_k[j];
                    gid_out[dst] = st_g[j];
                    slot_out[dst] = st_s[j];
                }
            }
        }
        r0 = r1;
    }
}

// The partition and the finish of the cells plan on the ping-pong buffers of the one-sweep passes (launch_onesweep_partition): the last
// kernel writes the buffers the layout calls point_list and slot_list, *keys_final names the keys that went with them.
int launch_cell_sort(int64_t cap, const Buffers &v, uint32_t **keys_final, uint32_t *host_late, uint32_t tag,
                     uint32_t *host_flag, uint32_t flag_value, bool debug, hipStream_t s) {
    if (v.L.part_passes > 2 || v.L.kbits != 8 * v.L.part_passes || v.L.dbits < 1 || v.L.dbits > 7) {
        set_error("the cells plan needs a partition key of 8 or 16 bits with depth buckets (kbits %d, dbits %d, passes %d)", v.L.kbits, v.L.dbits, v.L.part_passes);
        return DAS3R_ERR_INVALID_ARG;
    }
    const uint32_t *n_ptr = v.g_count();
    uint32_t *err = v.err_word();
    uint32_t *keyA = v.b_keyA(), *keyB = v.b_keyB();
    uint32_t *gid_of = v.b_gid_of(), *slot_list = v.b_slot(), *e_tmp = v.b_e2();
    uint32_t *ghist = v.b_ghist(), *cursor = v.b_cursor();
    uint32_t *const pl_final = v.point_list(), *const pl_other = v.point_list_partner();
    uint2 *ranges = v.ranges();
    const bool two = v.L.part_passes == 2;
    if (two) {
        const int ipl = sort_items_per_lane(cap);
        const int nblocks = div_up(cap, (int64_t)256 * ipl);
#define PART(IPL)                                                                                                                      \
    DAS3R_LAUNCH((cell_partition_kernel<IPL>), dim3(nblocks), dim3(256), 0, s, keyA, gid_of, keyB, pl_other, e_tmp, (uint32_t)cap, n_ptr, \
                 v.L.kshift + 8, ghist + 256, cursor, v.L.cursor_stride, err)
        if (ipl == 4) PART(4); else if (ipl == 8) PART(8); else PART(16);
#undef PART
        KERNEL_CHECK(s, debug, "cell_partition");
    }
    const uint32_t ncells = two ? (((uint32_t)v.L.ntiles - 1u) >> (8 - v.L.dbits)) + 1u : 1u;
    const uint32_t grid = ((ncells + 7u) & ~7u) * (uint32_t)CELL_SPLIT;
    uint32_t *kout = two ? keyA : keyB;
    DAS3R_LAUNCH(cell_finish_kernel, dim3(grid), dim3(256), 0, s, two ? keyB : keyA, two ? pl_other : gid_of, two ? e_tmp : (uint32_t *)nullptr, kout,
                 pl_final, slot_list, (uint32_t)cap, n_ptr, v.L.kshift, v.L.dbits, (uint32_t)v.L.ntiles, ncells, two ? ghist + 256 : (uint32_t *)nullptr,
                 two ? cursor : (uint32_t *)nullptr, v.L.cursor_stride, ranges, err, host_late, tag, (uint32_t)switches().inject_fault, host_flag, flag_value);
    KERNEL_CHECK(s, debug, "cell_finish");
    *keys_final = kout;
    return DAS3R_OK;
}

}  // namespace das3r
