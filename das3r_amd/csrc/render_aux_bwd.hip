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
// The walk is render_lists.h's back-to-front one (walk_list_back_to_front: the batches reversed, the two-half column flush, the rows of
// unreached entries zeroed), every pixel starting at T = final_T[pixel].  Per (wave, entry) it reduces the six moments + up to 2 feature
// sums in one transposed pass, the other feature sums in a second — a single ninth value, C = 3, on a DPP chain instead.
//
// With FEAT the same walk also leaves w dL_dout[c] (w = alpha T) per instance in a second [capacity, C] row array, which render_aux.hip's
// aux_gather_kernel reduces to dL_dfeatures: one walk gives both gradients.
//
// LDS at C = 8 with FEAT is 17 KB of staged entries + 28 KB of columns = 45 KB, three workgroups per CU (160 KB); at C = 3 with FEAT 30 KB,
// five.  One workgroup per tile only: few tiles with long lists (the DAS3R training shape) leave CUs idle — a bucket-parallel form, as the
// adjoint has, is owed (docs/ledger.md (ck)).
#include "render_lists.h"

namespace das3r {

template <int C, bool FEAT>
__global__ void __launch_bounds__(256) render_aux_backward_kernel(const ListArgs a, const float *__restrict__ feat /*[P,C]; C > 0*/,
                                                                  const float *__restrict__ dL_dout /*[C,H,W]; C > 0*/,
                                                                  const float *__restrict__ dL_dalpha /*[H,W] or null*/, float *__restrict__ partial /*[capacity,9]*/,
                                                                  float *__restrict__ partial_f /*[capacity,C]; FEAT*/) {
    static_assert(!(FEAT && C == 0), "feature rows need a channel");
    constexpr int CF = C > 0 ? C : 1;
    constexpr int NV = 6 + (FEAT ? C : 0);   // values per (wave, entry): the six moments, then w dL_dout[c]
    __shared__ float4 s_xyh[TILE_PIX], s_co[TILE_PIX];
    __shared__ float s_f[TILE_PIX * CF];     // row j = the feature row of staged entry j (wave-uniform reads: broadcasts)
    __shared__ uint32_t s_slot[TILE_PIX];
    __shared__ WaveColumns<NV> wc;

    const TileLane t = tile_lane(a, blockIdx.x, threadIdx.x >> 6);
    if (t.tile < 0) return;
    const size_t plane = (size_t)a.H * a.W;
    const float T_final = t.inside ? a.final_T[t.pix] : 0.f;
    float g[CF];
#pragma unroll
    for (int c = 0; c < CF; c++) g[c] = (C > 0 && t.inside) ? dL_dout[(size_t)c * plane + t.pix] : 0.f;
    // 1 - final_T takes dL_dalpha: d/dalpha_k of it is T_final / (1 - alpha_k) — replay_pair's background slot with the sign turned
    const float tfbg = (dL_dalpha != nullptr && t.inside) ? -T_final * dL_dalpha[t.pix] : 0.f;

    ReplayState st = {T_final, 0.f};
    walk_list_back_to_front<NV, false, (FEAT ? C : 0)>(
        a, t, s_xyh, s_co, s_slot, wc, partial, partial_f,
        [&](const int j, const uint32_t gi) {
#pragma unroll
            for (int c = 0; c < C; c++) s_f[j * CF + c] = feat[(size_t)gi * C + c];
        },
        [&](const int j, uint32_t, const bool active, const float alpha, const float G, const float dx, const float dy) {
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
            store_totals8(wc, j, a8, 0);
            if constexpr (FEAT && C == 3) {
                // nine values: the ninth on a DPP chain (its total in lane 63), as the colour backward reduces its ninth
                const float r1 = wave_sum_to_lane63(v[0] * g[2]);
                if (__lane_id() == 63) wc.col[threadIdx.x >> 6][(j & (LIST_HALF - 1)) * NV + 8] = r1;
            } else if constexpr (FEAT && C > 3) {
                float b8[8];
#pragma unroll
                for (int q = 0; q < 8; q++) b8[q] = (q + 2 < C) ? v[0] * g[q + 2 < C ? q + 2 : 0] : 0.f;
                store_totals8(wc, j, b8, 8);
            }
        });
}

// (FEAT instantiations only where there are feature rows to write: C > 0 and partial_f given)
#define AUXB_LAUNCH(N, FEAT) \
    DAS3R_LAUNCH((render_aux_backward_kernel<N, FEAT>), dim3(xcd_grid(v.L)), dim3(TILE_PIX), 0, s, lists, feat, dL_dout, dL_dalpha, partial, partial_f)
#define AUXB_CASE(N)                                  \
    case N:                                           \
        if (N > 0 && partial_f) AUXB_LAUNCH(N, (N > 0)); \
        else AUXB_LAUNCH(N, false);                   \
        break;

// partial: [capacity, 9] rows for launch_preprocess_backward; partial_f: [capacity, C] rows for aux_gather_kernel, or null (no dL_dfeatures)
int launch_render_aux_backward(int P, int W, int H, int C, const float *feat, const float *dL_dout, const float *dL_dalpha, float *partial,
                               float *partial_f, const Buffers &v, bool debug, hipStream_t s) {
    const ListArgs lists = list_args(v, W, H, P);
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
    KERNEL_CHECK(s, debug, "render_aux_backward");
    return DAS3R_OK;
}

}  // namespace das3r
