// render_distort.hip — the ray-distortion regulariser over the lists a forward has left behind, forward and compositing backward
// (include/das3r_raster.h das3r_raster_distortion_forward / das3r_raster_distortion_backward: the definition is fixed there, word for word).
//
//     D[pixel] = sum_{j<k} w_j w_k (m_j - m_k) = sum_k w_k (B_{k-1} - m_k A_{k-1}),     w_k = alpha_k T_k,  m_k = 1 / z_k,
//     A_k = sum_{j<=k} w_j,  B_k = sum_{j<=k} w_j m_j
//
// over the list positions k < n_contrib[pixel] — the colour's own entries, order, alpha (pair_alpha) and stop; no background term.  The
// lists are in (depth, index) order, so every term is >= 0.  Quadratic in the weights: no blend of per-Gaussian channels (render_aux.hip)
// gives it.
//
// The shift.  D does not change under m -> m + c, and B - m A cancels in fp32 unless m is taken relative to something near the pixel's own
// depths.  The reference here is PER PIXEL and is the WEIGHTED MEAN mu = B / A of the inverse depths themselves — a fixed entry's 1/z (the
// tile's or the pixel's first) fails when that entry is an outlier: a faint splat just past the near plane in front of a distant surface
// (tests' `culled` scene: 1/z = 909 before 0.2) leaves every later difference with the rounding of 909.  The forward carries mu as a running
// mean, B_{k-1} - m_k A_{k-1} = A_{k-1} (mu_{k-1} - m_k) with mu_k = mu_{k-1} + w_k (m_k - mu_{k-1}) / A_k (one v_rcp_f32 per pair): every
// difference is taken between actual inverse depths.  The backward takes m relative to the pixel's FINAL mean, the shift in which the total
// B is zero.
//
// Forward (render_distortion_forward_kernel): render_aux.hip's tile kernel with three running values (A, mu, D) in place of the channel sums:
// one 256-lane workgroup per 16x16 tile, a wave per 8x8 quadrant, the list staged through LDS in batches of 256 with 1/z alongside, a ballot
// cull per quadrant.  It writes D [H,W] and — THE CHOSEN DESIGN for the backward's total, the totals plane — the pixel's final mu = B / A
// [H,W] into caller memory (null: not wanted): the total B in the form the backward needs it, the shift that makes it vanish.  A first
// contributor meets A = 0: an empty pixel and a pixel with one contributor are exactly 0.
//
// Backward (render_distortion_backward_kernel): render_aux_bwd.hip's decomposition — the batch order reversed, every pixel starting at
// T = final_T, pair_alpha, then replay_pair_moments on the per-pair scalar
//     cd = dL_dD[pixel] q_k,     q_k = dD/dw_k = m_k (2 SA_k - A) - (2 SB_k - B),     SA_k = sum_{j>k} w_j,  SB_k = sum_{j>k} w_j m_j
// (dD/dalpha_k = T_k q_k - (sum_{j>k} w_j q_j) / (1 - alpha_k): the colour recurrence), SA and SB carried as running sums of the replay,
// A = 1 - final_T, m_k := 1/z_k - mu[pixel] with mu read from the totals plane and hence B = 0: no front-to-back sweep here.  The depth
// gradient is one more value per pair,
//     dL_dD[pixel] dD/dm_k = dL_dD[pixel] w_k (2 SA_k + w_k - A),
// reduced with the six moments in ONE transposed wave reduction (seven of its eight values), every wave storing its totals into its own LDS
// column, the four columns added in the order 0, 1, 2, 3 (a column that was not stored counts as 0: a select, nothing is zeroed), the row
// written into the entry's emission slot: column 0 the dL/dm sum, columns 1..2 zero, 3..8 replay_pair's geometry sums.  Zeros for list entries
// no pixel reaches: nothing needs pre-zeroing.  No floating-point atomics, no unordered LDS adds: bit-identical from run to run.
//
// distortion_fold_kernel then adds a Gaussian's column-0 sums (rows e0 .. e0 + tiles_touched - 1: its alone) into dz[i] = -s / z^2 in caller
// scratch and zeroes the column, so that the per-Gaussian backward reads a zero colour gradient.
//
// One workgroup per tile in both kernels, accepted as for the aux backward: few tiles with long lists leave CUs idle.  The bucket-parallel
// form is owed: a list segment started from T = 1 composes associatively on (T, A, B, D), B = mu A —
//     (T, A, B, D) o (T', A', B', D') = (T T', A + T A', B + T B', D + T^2 D' + T (B A' - A B')),     B A' - A B' = A A' (mu - mu')
// (docs/ledger.md (cq)).
#include "render_common.h"

namespace das3r {

// 1/z of a splat record's depth: the forwards' staged_invz
__device__ __forceinline__ float record_invz(const float4 *__restrict__ rgbd, const uint32_t g) { return 1.0f / rgbd[(size_t)g * SPLAT_REC].w; }

__global__ void __launch_bounds__(256) render_distortion_forward_kernel(
    const uint2 *__restrict__ ranges, const uint32_t *__restrict__ point_list, int W, int H, int tiles_x, int ntiles_strip /*render_common.h pack_tiles*/,
    const float4 *__restrict__ xyh, const float4 *__restrict__ conic_opacity, const float4 *__restrict__ rgbd, const uint32_t *__restrict__ n_contrib,
    float *__restrict__ out /*[H,W]*/, float *__restrict__ totals /*[H,W] or null*/, uint32_t last_g, uint32_t cap) {
    __shared__ float4 s_xyh[TILE_PIX], s_co[TILE_PIX];
    __shared__ float s_m[TILE_PIX];   // 1/z of staged entry j (wave-uniform reads: broadcasts)
    __shared__ uint32_t s_max[4];

    const int tile = xcd_tile(blockIdx.x, ntiles_strip, tiles_x);
    if (tile < 0) return;
    const int tid = threadIdx.x, lane = __lane_id(), wave = tid >> 6;
    const int bx = tile % tiles_x, by = tile / tiles_x;
    int px, py;
    quadrant_pixel(bx, by, wave, lane, px, py);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    const float qcx = (float)(bx * TILE_X + ((wave & 1) << 3)) + 3.5f, qcy = (float)(by * TILE_Y + ((wave >> 1) << 3)) + 3.5f;
    const uint2 range = safe_range(ranges[tile], cap);
    const size_t pix = (size_t)py * W + px;
    const uint32_t last_contributor = inside ? n_contrib[pix] : 0u;

    // no pixel of the tile blended anything past list position max_contrib; no pixel of this wave past wmax
    uint32_t wmax = last_contributor;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, o, 64));
    if (lane == 0) s_max[wave] = wmax;
    __syncthreads();
    const uint32_t max_contrib = min(max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])), range.y - range.x);
    const int rounds = ((int)max_contrib + TILE_PIX - 1) / TILE_PIX;

    float T = 1.0f, A = 0.f, mu = 0.f, D = 0.f;
    for (int i = 0; i < rounds; i++) {
        const int done_before = i * TILE_PIX;
        const int n = min(TILE_PIX, (int)max_contrib - done_before);
        if (i > 0) __syncthreads();   // the previous batch has been read by every wave
        if (tid < n) {
            const uint32_t g = min(point_list[range.x + done_before + tid], last_g);
            s_xyh[tid] = xyh[(size_t)g * SPLAT_REC];
            s_co[tid] = conic_opacity[(size_t)g * SPLAT_REC];
            s_m[tid] = record_invz(rgbd, g);
        }
        __syncthreads();
        if ((uint32_t)done_before >= wmax) continue;   // (wave-uniform; the barriers above are still taken by every wave)
        uint64_t masks[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int s = k * 64 + lane;
            masks[k] = __ballot(s < n && quadrant_hit(s_xyh[s], qcx, qcy));
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint64_t m = masks[k];
            while (m != 0ull) {
                const int j = k * 64 + __builtin_ctzll(m);
                m &= m - 1ull;
                const uint32_t position = (uint32_t)(done_before + j);   // 0-based list position
                if (position >= wmax) break;                             // (uniform: the bits come in list order)
                const float4 p = s_xyh[j];
                const float4 co = s_co[j];
                float dx, dy, G, alpha;
                const bool active = pair_alpha(p.x, p.y, co, pxf, pyf, dx, dy, G, alpha) & (position < last_contributor);
                if (__ballot(active) == 0ull) continue;
                const float a = active ? alpha : 0.f;
                const float w = a * T, d = s_m[j] - mu;            // m_k - mu_{k-1}
                D = __fmaf_rn(-w, A * d, D);                         // w_k (B_{k-1} - m_k A_{k-1}) = w_k A_{k-1} (mu_{k-1} - m_k)
                // mu_k = mu_{k-1} + r (m_k - mu_{k-1}),  r = w_k / A_k — exactly 1 for the first contributor and never above it, so that mu stays
                // on the near side of every later m and no term turns negative by a rounding; w = 0: mu unchanged
                const float Anew = A + w;
                const float r = A > 0.f ? fminf(w * __builtin_amdgcn_rcpf(Anew), 1.0f) : (w > 0.f ? 1.0f : 0.f);
                A = Anew;
                mu = __fmaf_rn(r, d, mu);
                T = T * (1.0f - a);
            }
        }
    }
    if (inside) {
        out[pix] = D;
        if (totals != nullptr) totals[pix] = mu;
    }
}

__global__ void __launch_bounds__(256) render_distortion_backward_kernel(
    const uint2 *__restrict__ ranges, const uint32_t *__restrict__ point_list, int W, int H, int tiles_x, int ntiles_strip /*render_common.h pack_tiles*/,
    const float4 *__restrict__ xyh, const float4 *__restrict__ conic_opacity, const float4 *__restrict__ rgbd, const uint32_t *__restrict__ n_contrib,
    const float *__restrict__ final_T, const float *__restrict__ dL_ddist /*[H,W]*/, const float *__restrict__ totals /*[H,W]: the forward kernel's mu*/,
    const uint32_t *__restrict__ slot_list, float *__restrict__ partial /*[capacity,9]*/, uint32_t last_g, uint32_t cap) {
    constexpr int NV = 7;   // values per (wave, entry): the six moments, then the dL/dm sum
    __shared__ float4 s_xyh[TILE_PIX], s_co[TILE_PIX];
    __shared__ float s_m[TILE_PIX];              // 1/z of staged entry j
    __shared__ uint32_t s_slot[TILE_PIX];        // emission slot of every staged entry = its row of `partial`
    constexpr int HALF = TILE_PIX / 2;           // the staged batch is walked and flushed in two halves: half the column storage
    __shared__ float col[4][HALF * NV];          // col[wave][jl * NV + q]: the wave's total of value q for entry jl of the half, where it stored one
    __shared__ unsigned long long s_vis[4][2];   // s_vis[wave][kk] bit b: the wave stored its totals for entry 64 kk + b of the half
    __shared__ uint32_t s_max[4];

    const int tile = xcd_tile(blockIdx.x, ntiles_strip, tiles_x);
    if (tile < 0) return;
    const int tid = threadIdx.x, lane = __lane_id(), wave = tid >> 6;
    const int bx = tile % tiles_x, by = tile / tiles_x;
    int px, py;
    quadrant_pixel(bx, by, wave, lane, px, py);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    const float qcx = (float)(bx * TILE_X + ((wave & 1) << 3)) + 3.5f, qcy = (float)(by * TILE_Y + ((wave >> 1) << 3)) + 3.5f;
    const uint2 range = safe_range(ranges[tile], cap);
    const size_t pix = (size_t)py * W + px;
    const uint32_t last_contributor = inside ? n_contrib[pix] : 0u;
    const float T_final = inside ? final_T[pix] : 0.f;
    const float gD = inside ? dL_ddist[pix] : 0.f;
    // A = 1 - final_T; m is taken relative to the pixel's mean mu = B / A (the totals plane), where the total B is zero
    const float Atot = inside ? 1.0f - T_final : 0.f, mu = inside ? totals[pix] : 0.f;
    const float ddelx_dx = 0.5f * W, ddely_dy = 0.5f * H;

    // no pixel of the tile blended anything past list position max_contrib, no pixel of this wave past wmax: the replay starts there
    uint32_t wmax = last_contributor;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, o, 64));
    if (lane == 0) s_max[wave] = wmax;
    __syncthreads();
    const uint32_t len = range.y - range.x;
    const uint32_t max_contrib = min(max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3])), len);
    const int rounds = ((int)max_contrib + TILE_PIX - 1) / TILE_PIX;

    // list entries beyond them are reached by no pixel of this tile: their rows are zero (cap > 0 whenever a list has entries)
    {
        const uint32_t ntail = (len - max_contrib) * 9u;
        for (uint32_t f = tid; f < ntail; f += TILE_PIX) {
            const uint32_t t = f / 9u, q = f - t * 9u;
            partial[(size_t)min(slot_list[range.x + max_contrib + t], cap - 1u) * 9 + q] = 0.f;
        }
    }

    ReplayState st = {T_final, 0.f};
    float SA = 0.f, SB = 0.f;              // the weights behind the current entry, and their sum of w (1/z - mu)
    const bool writer = (lane & 7) == 0;   // after the transposed reduction lane l holds the total of value l >> 3
    const int widx = lane >> 3;

    for (int i = 0; i < rounds; i++) {
        const int done_before = i * TILE_PIX;
        const int n = min(TILE_PIX, (int)max_contrib - done_before);
        // the batch in reverse list order: staged entry j holds list position max_contrib - 1 - done_before - j
        if (tid < n) {
            const uint32_t pos = range.x + max_contrib - 1u - (uint32_t)done_before - (uint32_t)tid;
            const uint32_t gi = min(point_list[pos], last_g);
            s_slot[tid] = min(slot_list[pos], cap - 1u);
            s_xyh[tid] = xyh[(size_t)gi * SPLAT_REC];
            s_co[tid] = conic_opacity[(size_t)gi * SPLAT_REC];
            s_m[tid] = record_invz(rgbd, gi);
        }
        __syncthreads();

        // the batch's positions are max_contrib - done_before - n .. max_contrib - done_before - 1: all at or past this wave's last one?
        const bool wave_in = max_contrib - (uint32_t)done_before - (uint32_t)n < wmax;   // (wave-uniform; the barriers are taken by every wave)
        uint64_t masks[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int s = k * 64 + lane;
            masks[k] = wave_in ? __ballot(s < n && quadrant_hit(s_xyh[s], qcx, qcy)) : 0ull;
        }
        // walked and flushed in two halves of 128 entries: the columns are half the size, the walk's order is the same
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (h * HALF >= n) continue;   // (uniform over the workgroup: n is)
            const int nh = min(HALF, n - h * HALF);
            unsigned long long vis[2] = {0ull, 0ull};   // (wave-uniform)
#pragma unroll
            for (int kk = 0; kk < 2; kk++) {
                uint64_t m = masks[2 * h + kk];
                while (m != 0ull) {
                    const int b = __builtin_ctzll(m), jl = kk * 64 + b, j = h * HALF + jl;
                    m &= m - 1ull;
                    const uint32_t position = max_contrib - 1u - (uint32_t)done_before - (uint32_t)j;   // 0-based list position, descending
                    if (position >= wmax) continue;                                                    // (uniform)
                    const float4 p = s_xyh[j];
                    const float4 co = s_co[j];
                    float dx, dy, G, alpha;
                    const bool active = pair_alpha(p.x, p.y, co, pxf, pyf, dx, dy, G, alpha) & (position < last_contributor);
                    if (__ballot(active) == 0ull) continue;   // (uniform) nobody's state changes: the entry's column stays unstored = 0
                    const float mk = s_m[j] - mu;
                    // q_k = m_k (2 SA_k - A) - (2 SB_k - B),  B = 0
                    const float qk = __fmaf_rn(mk, __fmaf_rn(2.0f, SA, -Atot), -2.0f * SB);
                    // replay_pair's recurrence on the one scalar cd = dL_dD q_k (colour (cd, 0, 0) against dL/dpix (1, 0, 0)): v[0] = w = alpha T,
                    // v[3..8] the six moments
                    float v[9];
                    replay_pair_moments(active, alpha, G, dx, dy, make_float4(gD * qk, 0.f, 0.f, 0.f), 1.0f, 0.f, 0.f, 0.f, st, v);
                    const float w = v[0];
                    float a8[8];
#pragma unroll
                    for (int q = 0; q < 6; q++) a8[q] = v[3 + q];
                    // dL_dD dD/dm_k = dL_dD w_k (2 SA_k + w_k - A) = dL_dD w_k (SA_k - F_k), F_k = A - w_k - SA_k the weights in front of k.
                    // F_k is known to no better than 2^-22: A = 1 - final_T carries the rounding of 1 - alpha (half an ulp of 1), w_k the ulp
                    // of the reciprocal that rebuilt T.  Below that it is taken as the zero it cannot be told from — so that a pixel's first
                    // contributor has nothing in front of it, and a pixel with one contributor sends exactly nothing.
                    float front = (Atot - w) - SA;
                    front = fabsf(front) < 0x1p-22f ? 0.f : front;
                    a8[6] = gD * (w * (SA - front));
                    a8[7] = 0.f;
                    SA = SA + w;
                    SB = __fmaf_rn(w, mk, SB);
                    const float r0 = wave_reduce8_transposed(a8, lane);
                    if (writer && widx < NV) col[wave][jl * NV + widx] = r0;   // a plain store: (wave, entry) pairs are visited once
                    vis[kk] |= 1ull << b;
                }
            }
            if (lane < 2) s_vis[wave][lane] = lane == 0 ? vis[0] : vis[1];
            __syncthreads();

            // the four waves' totals in a fixed order -> the rows of the entry's emission slot
            if (tid < nh) {
                const int kk = tid >> 6, b = tid & 63, j = h * HALF + tid;
                const bool have0 = (s_vis[0][kk] >> b) & 1ull, have1 = (s_vis[1][kk] >> b) & 1ull, have2 = (s_vis[2][kk] >> b) & 1ull,
                           have3 = (s_vis[3][kk] >> b) & 1ull;
                float mo[NV];
#pragma unroll
                for (int q = 0; q < NV; q++) {
                    const int f = tid * NV + q;
                    mo[q] = (((have0 ? col[0][f] : 0.f) + (have1 ? col[1][f] : 0.f)) + (have2 ? col[2][f] : 0.f)) + (have3 ? col[3][f] : 0.f);
                }
                // moments -> replay_pair's sums (render_common.h moments_to_sums), once per (tile, splat)
                const float4 co = s_co[j];
                const float hd = -0.5f * co.w;
                float *row = partial + (size_t)s_slot[j] * 9;
                row[0] = mo[6];   // the instance's dL/dm sum: distortion_fold_kernel takes it and leaves a zero
                row[1] = 0.f;
                row[2] = 0.f;
                row[3] = hd * (co.x * mo[0] + co.y * mo[1]) * (2.0f * ddelx_dx);
                row[4] = hd * (co.z * mo[1] + co.y * mo[0]) * (2.0f * ddely_dy);
                row[5] = hd * mo[2];
                row[6] = hd * mo[3];
                row[7] = hd * mo[4];
                row[8] = mo[5];
            }
            __syncthreads();   // before the columns are stored again, and before the next batch is staged over this one
        }
    }
}

// per splat: column 0 of its rows e0 .. e0 + tiles_touched - 1 (its alone: no atomics) is the sum over pixels of dL/dm; m = 1/z, so
// dz[i] = -s / z^2 (preprocess_bwd.hip depth_fold_kernel's step).  The column is left zero: the per-Gaussian backward reads columns 0..2 as
// the colour sums, and this loss has no colour gradient.
__global__ void __launch_bounds__(256) distortion_fold_kernel(int P, const uint32_t *__restrict__ tiles_touched, const uint32_t *__restrict__ off_by_gid,
                                                              const float4 *__restrict__ rgbd, float *__restrict__ partial, float *__restrict__ dz,
                                                              uint32_t cap) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t n = tiles_touched[i];
    float s = 0.f;
    if (n > 0u) {
        const uint32_t e0 = min(off_by_gid[i], cap), e1 = min(e0 + min(n, cap), cap);   // (kept inside the scratch whatever a failed binning left)
        for (uint32_t e = e0; e < e1; e++) {
            s += partial[(size_t)e * 9];
            partial[(size_t)e * 9] = 0.f;
        }
    }
    const float z = rgbd[(size_t)i * SPLAT_REC].w;
    dz[i] = n > 0u ? -s / (z * z) : 0.f;
}

#define DISTORT_LISTS                                                                                                     \
    (const uint2 *)(img + L.pub.ranges), (const uint32_t *)(binning + L.pub.point_list), W, H, L.tiles_x, pack_tiles(L),  \
        (const float4 *)(geom + L.pub.xy), (const float4 *)(geom + L.pub.conic_opacity), (const float4 *)(geom + L.pub.rgbd), \
        (const uint32_t *)(img + L.pub.n_contrib)

int launch_render_distortion_forward(int P, int W, int H, float *out, float *totals, const char *geom, const char *binning, const char *img,
                                     const Layout &L, bool debug, hipStream_t s) {
    DAS3R_LAUNCH(render_distortion_forward_kernel, dim3(xcd_grid(L)), dim3(TILE_PIX), 0, s, DISTORT_LISTS, out, totals, (uint32_t)(P - 1),
                 (uint32_t)L.capacity);
    KERNEL_CHECK(s, debug, "render_distortion_forward");
    return DAS3R_OK;
}

int launch_render_distortion_backward(int P, int W, int H, const float *dL_ddist, const float *totals, float *partial, const char *geom,
                                      const char *binning, const char *img, const Layout &L, bool debug, hipStream_t s) {
    DAS3R_LAUNCH(render_distortion_backward_kernel, dim3(xcd_grid(L)), dim3(TILE_PIX), 0, s, DISTORT_LISTS, (const float *)(img + L.pub.final_T),
                 dL_ddist, totals, (const uint32_t *)(binning + L.b_slot), partial, (uint32_t)(P - 1), (uint32_t)L.capacity);
    KERNEL_CHECK(s, debug, "render_distortion_backward");
    return DAS3R_OK;
}

int launch_distortion_fold(int P, const char *geom, const Layout &L, float *partial, float *dz, bool debug, hipStream_t s) {
    DAS3R_LAUNCH(distortion_fold_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, P, (const uint32_t *)(geom + L.pub.tiles_touched),
                 (const uint32_t *)(geom + L.g_off_by_gid), (const float4 *)(geom + L.pub.rgbd), partial, dz, (uint32_t)L.capacity);
    KERNEL_CHECK(s, debug, "distortion_fold");
    return DAS3R_OK;
}

}  // namespace das3r
