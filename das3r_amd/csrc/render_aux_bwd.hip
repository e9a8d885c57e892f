// render_aux_bwd.hip — the compositing backward of the aux channels and of the coverage image WITH RESPECT TO THE GEOMETRY
// (include/das3r_raster.h das3r_raster_aux_backward).
//
// render_aux.hip blends a caller's rows over a forward's saved lists with the geometry held constant.  This kernel is the other half: for
//     L = <dL_dout, aux image> + <dL_dalpha, 1 - final_T>             (either term may be absent)
// it replays every pixel back to front and leaves, per (tile, splat) instance, the six geometry sums of render_common.h replay_pair —
// dL/d(mean2D, conic, opacity) — in the nine-float row of the entry's emission slot, columns 0..2 (the colour sums) zero: exactly what
// launch_preprocess_backward consumes, so the per-Gaussian chain rule (and the antialiasing factor's derivative) is the colour loss's own.
//
// The recurrence is replay_pair's two scalars, T and R = sum over the splats behind of cd_j alpha_j T_j, with
//     cd = sum_c f[g][c] dL_dout[c][pixel]                              (a C-term dot product instead of rgb . dL/dpix)
// and no background term.  The coverage term enters in the DIRECT form  dL/dalpha_k += dL_dalpha[pixel] T_final / (1 - alpha_k) — replay_pair's
// tfbg slot with tfbg = -T_final dL_dalpha — never as a constant-one channel, whose T_k - R / (1 - alpha_k) cancels down to the same value
// and loses it in fp32 on deep pixels (docs/ledger.md (ck)).
//
// Decomposition of render_aux.hip's kernels with the batch order reversed: one 256-lane workgroup per 16x16 tile, a wave per 8x8 quadrant,
// the list staged through LDS in batches of 256 with the feature rows alongside, a ballot cull per quadrant, a pixel taking part in list
// position k iff k < n_contrib[pixel], every pixel starting at T = final_T[pixel]; alpha is pair_alpha's.
//
// Reductions: the 64 pixels of a wave on the cross-lane network (the transposed reduction: 6 moments + up to 2 feature sums in one pass,
// the other feature sums in a second — a single ninth value, C = 3, on a DPP chain instead), every wave STORING its totals into its own
// LDS column — a (wave, entry) pair is visited at most once per batch — and remembering which entries it stored in a 128-bit mask; the
// four columns are then added in the order 0, 1, 2, 3, a column
// that was not stored counting as 0 (a select: what the LDS held before does not matter, and no column needs zeroing).  No floating-point
// atomics, no unordered LDS adds: bit-identical from run to run.  The moments become replay_pair's sums once per (tile, splat)
// (moments_to_sums' arithmetic).
//
// With FEAT the same walk also leaves w dL_dout[c] (w = alpha T) per instance in a second [capacity, C] row array, which render_aux.hip's
// aux_gather_kernel reduces to dL_dfeatures: one walk gives both gradients.
//
// Every row of both arrays that belongs to a list entry of the tile is written — zeros for the entries no pixel reaches — so neither needs
// initialising.  The 256 staged entries are walked and flushed in two halves of 128, which halves the columns: LDS at C = 8 with FEAT is 17 KB
// of staged entries + 28 KB of columns = 45 KB, three workgroups per CU (160 KB); at C = 3 with FEAT 30 KB, five.  One workgroup per tile only: few tiles with long lists (the DAS3R training shape) leave CUs idle — a
// bucket-parallel form, as the adjoint has, is owed (docs/ledger.md (ck)).
#include "render_common.h"

namespace das3r {

template <int C, bool FEAT>
__global__ void __launch_bounds__(256) render_aux_backward_kernel(
    const uint2 *__restrict__ ranges, const uint32_t *__restrict__ point_list, int W, int H, int tiles_x, int ntiles_strip /*render_common.h pack_tiles*/,
    const float4 *__restrict__ xyh, const float4 *__restrict__ conic_opacity, const uint32_t *__restrict__ n_contrib, const float *__restrict__ final_T,
    const float *__restrict__ feat /*[P,C]; C > 0*/, const float *__restrict__ dL_dout /*[C,H,W]; C > 0*/, const float *__restrict__ dL_dalpha /*[H,W] or null*/,
    const uint32_t *__restrict__ slot_list, float *__restrict__ partial /*[capacity,9]*/, float *__restrict__ partial_f /*[capacity,C]; FEAT*/,
    uint32_t last_g, uint32_t cap) {
    static_assert(!(FEAT && C == 0), "feature rows need a channel");
    constexpr int CF = C > 0 ? C : 1;
    constexpr int NV = 6 + (FEAT ? C : 0);   // values per (wave, entry): the six moments, then w dL_dout[c]
    __shared__ float4 s_xyh[TILE_PIX], s_co[TILE_PIX];
    __shared__ float s_f[TILE_PIX * CF];         // row j = the feature row of staged entry j (wave-uniform reads: broadcasts)
    __shared__ uint32_t s_slot[TILE_PIX];        // emission slot of every staged entry = its row of `partial` / `partial_f`
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
    const size_t pix = (size_t)py * W + px, plane = (size_t)H * W;
    const uint32_t last_contributor = inside ? n_contrib[pix] : 0u;
    const float T_final = inside ? final_T[pix] : 0.f;
    float g[CF];
#pragma unroll
    for (int c = 0; c < CF; c++) g[c] = (C > 0 && inside) ? dL_dout[(size_t)c * plane + pix] : 0.f;
    // 1 - final_T takes dL_dalpha: d/dalpha_k of it is T_final / (1 - alpha_k) — replay_pair's background slot with the sign turned
    const float tfbg = (dL_dalpha != nullptr && inside) ? -T_final * dL_dalpha[pix] : 0.f;
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
        if constexpr (FEAT) {
            const uint32_t ntail_f = (len - max_contrib) * C;
            for (uint32_t f = tid; f < ntail_f; f += TILE_PIX) {
                const uint32_t t = f / C, q = f - t * C;
                partial_f[(size_t)min(slot_list[range.x + max_contrib + t], cap - 1u) * C + q] = 0.f;
            }
        }
    }

    ReplayState st = {T_final, 0.f};
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
#pragma unroll
            for (int c = 0; c < C; c++) s_f[tid * CF + c] = feat[(size_t)gi * C + c];
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
        // walked and flushed in two halves of 128 entries: the columns are half the size (occupancy), the walk's order is the same
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
                    float cd = 0.f;
#pragma unroll
                    for (int c = 0; c < C; c++) cd = __fmaf_rn(s_f[j * CF + c], g[c], cd);
                    // replay_pair's recurrence on the one scalar cd (colour (cd, 0, 0) against dL/dpix (1, 0, 0)): v[0] = w = alpha T,
                    // v[3..8] the six moments
                    float v[9];
                    replay_pair_moments(active, alpha, G, dx, dy, make_float4(cd, 0.f, 0.f, 0.f), 1.0f, 0.f, 0.f, tfbg, st, v);
                    float a8[8];
#pragma unroll
                    for (int q = 0; q < 6; q++) a8[q] = v[3 + q];
                    a8[6] = (FEAT && C > 0) ? v[0] * g[0] : 0.f;
                    a8[7] = (FEAT && C > 1) ? v[0] * g[C > 1 ? 1 : 0] : 0.f;
                    const float r0 = wave_reduce8_transposed(a8, lane);
                    if (writer && widx < (NV < 8 ? NV : 8)) col[wave][jl * NV + widx] = r0;   // a plain store: (wave, entry) pairs are visited once
                    if constexpr (FEAT && C == 3) {
                        // nine values: the ninth on a DPP chain (its total in lane 63), as the colour backward reduces its ninth
                        const float r1 = wave_sum_to_lane63(v[0] * g[2]);
                        if (lane == 63) col[wave][jl * NV + 8] = r1;
                    } else if constexpr (FEAT && C > 3) {
                        float b8[8];
#pragma unroll
                        for (int q = 0; q < 8; q++) b8[q] = (q + 2 < C) ? v[0] * g[q + 2 < C ? q + 2 : 0] : 0.f;
                        const float r1 = wave_reduce8_transposed(b8, lane);
                        if (writer && 8 + widx < NV) col[wave][jl * NV + 8 + widx] = r1;
                    }
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
                float mo[6];
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    const int f = tid * NV + q;
                    mo[q] = (((have0 ? col[0][f] : 0.f) + (have1 ? col[1][f] : 0.f)) + (have2 ? col[2][f] : 0.f)) + (have3 ? col[3][f] : 0.f);
                }
                // moments -> replay_pair's sums (render_common.h moments_to_sums), once per (tile, splat)
                const float4 co = s_co[j];
                const float hd = -0.5f * co.w;
                float *row = partial + (size_t)s_slot[j] * 9;
                row[0] = 0.f;
                row[1] = 0.f;
                row[2] = 0.f;
                row[3] = hd * (co.x * mo[0] + co.y * mo[1]) * (2.0f * ddelx_dx);
                row[4] = hd * (co.z * mo[1] + co.y * mo[0]) * (2.0f * ddely_dy);
                row[5] = hd * mo[2];
                row[6] = hd * mo[3];
                row[7] = hd * mo[4];
                row[8] = mo[5];
            }
            if constexpr (FEAT) {
                for (int f = tid; f < nh * C; f += TILE_PIX) {
                    const int jl = f / C, q = f - jl * C, kk = jl >> 6, b = jl & 63, e = jl * NV + 6 + q;
                    const float t0 = ((s_vis[0][kk] >> b) & 1ull) ? col[0][e] : 0.f, t1 = ((s_vis[1][kk] >> b) & 1ull) ? col[1][e] : 0.f;
                    const float t2 = ((s_vis[2][kk] >> b) & 1ull) ? col[2][e] : 0.f, t3 = ((s_vis[3][kk] >> b) & 1ull) ? col[3][e] : 0.f;
                    partial_f[(size_t)s_slot[h * HALF + jl] * C + q] = ((t0 + t1) + t2) + t3;
                }
            }
            __syncthreads();   // before the columns are stored again, and before the next batch is staged over this one
        }
    }
}

#define AUXB_CASE(N)                                                                                                                   \
    case N:                                                                                                                            \
        if (N > 0 && partial_f) DAS3R_LAUNCH((render_aux_backward_kernel<N, (N > 0)>), dim3(xcd_grid(L)), dim3(TILE_PIX), 0, s, AUXB_ARGS); \
        else DAS3R_LAUNCH((render_aux_backward_kernel<N, false>), dim3(xcd_grid(L)), dim3(TILE_PIX), 0, s, AUXB_ARGS);                 \
        break;

// partial: [capacity, 9] rows for launch_preprocess_backward; partial_f: [capacity, C] rows for aux_gather_kernel, or null (no dL_dfeatures)
int launch_render_aux_backward(int P, int W, int H, int C, const float *feat, const float *dL_dout, const float *dL_dalpha, float *partial,
                               float *partial_f, const char *geom, const char *binning, const char *img, const Layout &L, bool debug, hipStream_t s) {
#define AUXB_ARGS                                                                                                                      \
    (const uint2 *)(img + L.pub.ranges), (const uint32_t *)(binning + L.pub.point_list), W, H, L.tiles_x, pack_tiles(L),               \
        (const float4 *)(geom + L.pub.xy), (const float4 *)(geom + L.pub.conic_opacity), (const uint32_t *)(img + L.pub.n_contrib),    \
        (const float *)(img + L.pub.final_T), feat, dL_dout, dL_dalpha, (const uint32_t *)(binning + L.b_slot), partial, partial_f,    \
        (uint32_t)(P - 1), (uint32_t)L.capacity
    switch (C) {
        AUXB_CASE(0)
        AUXB_CASE(1)
        AUXB_CASE(2)
        AUXB_CASE(3)
        AUXB_CASE(4)
        AUXB_CASE(5)
        AUXB_CASE(6)
        AUXB_CASE(7)
        default:
        AUXB_CASE(8)
    }
#undef AUXB_ARGS
    KERNEL_CHECK(s, debug, "render_aux_backward");
    return DAS3R_OK;
}

}  // namespace das3r
