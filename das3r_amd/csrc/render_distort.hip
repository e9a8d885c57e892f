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
// Forward (render_distortion_forward_kernel): render_lists.h's front-to-back walk with 1/z staged alongside and three running values
// (A, mu, D).  It writes D [H,W] and — THE CHOSEN DESIGN for the backward's total, the totals plane — the pixel's final mu = B / A
// [H,W] into caller memory (null: not wanted): the total B in the form the backward needs it, the shift that makes it vanish.  A first
// contributor meets A = 0: an empty pixel and a pixel with one contributor are exactly 0.
//
// Backward (render_distortion_backward_kernel): render_lists.h's back-to-front walk, every pixel starting at T = final_T, with
// replay_pair_moments on the per-pair scalar
//     cd = dL_dD[pixel] q_k,     q_k = dD/dw_k = m_k (2 SA_k - A) - (2 SB_k - B),     SA_k = sum_{j>k} w_j,  SB_k = sum_{j>k} w_j m_j
// (dD/dalpha_k = T_k q_k - (sum_{j>k} w_j q_j) / (1 - alpha_k): the colour recurrence), SA and SB carried as running sums of the replay,
// A = 1 - final_T, m_k := 1/z_k - mu[pixel] with mu read from the totals plane and hence B = 0: no front-to-back sweep here.  The depth
// gradient is one more value per pair,
//     dL_dD[pixel] dD/dm_k = dL_dD[pixel] w_k (2 SA_k + w_k - A),
// reduced with the six moments in ONE transposed wave reduction (seven of its eight values) and written to column 0 of the entry's
// nine-float row: column 0 the dL/dm sum, columns 1..2 zero, 3..8 replay_pair's geometry sums.
//
// distortion_fold_kernel then adds a Gaussian's column-0 sums (rows e0 .. e0 + tiles_touched - 1: its alone) into dz[i] = -s / z^2 in caller
// scratch and zeroes the column, so that the per-Gaussian backward reads a zero colour gradient.
//
// One workgroup per tile in both kernels, accepted as for the aux backward: few tiles with long lists leave CUs idle.  The bucket-parallel
// form is owed: a list segment started from T = 1 composes associatively on (T, A, B, D), B = mu A —
//     (T, A, B, D) o (T', A', B', D') = (T T', A + T A', B + T B', D + T^2 D' + T (B A' - A B')),     B A' - A B' = A A' (mu - mu')
// (docs/ledger.md (cq)).
#include "render_lists.h"

namespace das3r {

// 1/z of a splat record's depth: the forwards' staged_invz
__device__ __forceinline__ float record_invz(const float4 *__restrict__ rgbd, const uint32_t g) { return 1.0f / rgbd[(size_t)g * SPLAT_REC].w; }

__global__ void __launch_bounds__(256) render_distortion_forward_kernel(const ListArgs a, float *__restrict__ out /*[H,W]*/, float *__restrict__ totals /*[H,W] or null*/) {
    __shared__ float4 s_xyh[TILE_PIX], s_co[TILE_PIX];
    __shared__ float s_m[TILE_PIX];   // 1/z of staged entry j (wave-uniform reads: broadcasts)

    const TileLane t = tile_lane(a, blockIdx.x, threadIdx.x >> 6);
    if (t.tile < 0) return;

    float T = 1.0f, A = 0.f, mu = 0.f, D = 0.f;
    walk_list_front_to_back(
        a, t, s_xyh, s_co, [&](const int j, const uint32_t g) { s_m[j] = record_invz(a.rgbd, g); },
        [&](const int j, uint32_t, const bool active, const float alpha, float, float, float) {
            const float al = active ? alpha : 0.f;
            const float w = al * T, d = s_m[j] - mu;           // m_k - mu_{k-1}
            D = __fmaf_rn(-w, A * d, D);                         // w_k (B_{k-1} - m_k A_{k-1}) = w_k A_{k-1} (mu_{k-1} - m_k)
            // mu_k = mu_{k-1} + r (m_k - mu_{k-1}),  r = w_k / A_k — exactly 1 for the first contributor and never above it, so that mu stays
            // on the near side of every later m and no term turns negative by a rounding; w = 0: mu unchanged
            const float Anew = A + w;
            const float r = A > 0.f ? fminf(w * __builtin_amdgcn_rcpf(Anew), 1.0f) : (w > 0.f ? 1.0f : 0.f);
            A = Anew;
            mu = __fmaf_rn(r, d, mu);
            T = T * (1.0f - al);
        });
    if (t.inside) {
        out[t.pix] = D;
        if (totals != nullptr) totals[t.pix] = mu;
    }
}

__global__ void __launch_bounds__(256) render_distortion_backward_kernel(const ListArgs a, const float *__restrict__ dL_ddist /*[H,W]*/,
                                                                         const float *__restrict__ totals /*[H,W]: the forward kernel's mu*/,
                                                                         float *__restrict__ partial /*[capacity,9]*/) {
    constexpr int NV = 7;   // values per (wave, entry): the six moments, then the dL/dm sum
    __shared__ float4 s_xyh[TILE_PIX], s_co[TILE_PIX];
    __shared__ float s_m[TILE_PIX];   // 1/z of staged entry j
    __shared__ uint32_t s_slot[TILE_PIX];
    __shared__ WaveColumns<NV> wc;

    const TileLane t = tile_lane(a, blockIdx.x, threadIdx.x >> 6);
    if (t.tile < 0) return;
    const float T_final = t.inside ? a.final_T[t.pix] : 0.f;
    const float gD = t.inside ? dL_ddist[t.pix] : 0.f;
    // A = 1 - final_T; m is taken relative to the pixel's mean mu = B / A (the totals plane), where the total B is zero
    const float Atot = t.inside ? 1.0f - T_final : 0.f, mu = t.inside ? totals[t.pix] : 0.f;

    ReplayState st = {T_final, 0.f};
    float SA = 0.f, SB = 0.f;   // the weights behind the current entry, and their sum of w (1/z - mu)
    // value 6, the instance's dL/dm sum, goes to column 0: distortion_fold_kernel takes it and leaves a zero
    walk_list_back_to_front<NV, true, 0>(
        a, t, s_xyh, s_co, s_slot, wc, partial, nullptr, [&](const int j, const uint32_t g) { s_m[j] = record_invz(a.rgbd, g); },
        [&](const int j, uint32_t, const bool active, const float alpha, const float G, const float dx, const float dy) {
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
            store_totals8(wc, j, a8, 0);
        });
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

int launch_render_distortion_forward(int P, int W, int H, float *out, float *totals, const Buffers &v, bool debug, hipStream_t s) {
    DAS3R_LAUNCH(render_distortion_forward_kernel, dim3(xcd_grid(v.L)), dim3(TILE_PIX), 0, s, list_args(v, W, H, P), out,
                 totals);
    KERNEL_CHECK(s, debug, "render_distortion_forward");
    return DAS3R_OK;
}

int launch_render_distortion_backward(int P, int W, int H, const float *dL_ddist, const float *totals, float *partial, const Buffers &v, bool debug, hipStream_t s) {
    DAS3R_LAUNCH(render_distortion_backward_kernel, dim3(xcd_grid(v.L)), dim3(TILE_PIX), 0, s, list_args(v, W, H, P),
                 dL_ddist, totals, partial);
    KERNEL_CHECK(s, debug, "render_distortion_backward");
    return DAS3R_OK;
}

int launch_distortion_fold(int P, const Buffers &v, float *partial, float *dz, bool debug, hipStream_t s) {
    DAS3R_LAUNCH(distortion_fold_kernel, dim3(div_up(P, 256)), dim3(256), 0, s, P, v.tiles_touched(),
                 v.g_off_by_gid(), v.rgbd(), partial, dz, (uint32_t)v.L.capacity);
    KERNEL_CHECK(s, debug, "distortion_fold");
    return DAS3R_OK;
}

}  // namespace das3r
