// render_aux.hip — compositing of a caller's per-Gaussian channels over the lists a forward has left behind, and its adjoint
// (include/das3r_raster.h das3r_raster_aux_forward / das3r_raster_aux_adjoint).
//
// The forward saves everything the blend needs: the tile ranges, the depth-ordered point list (the local-order kernels write their
// order back), every pixel's last contributor (n_contrib) and the 64-byte splat records (xy, conic + opacity: the antialiasing factor
// already folded into the opacity).  What differs from the colour kernels is the VALUE blended per splat: a row of a caller's
// [P, C] tensor instead of rgb.  No preprocess, no emission, no sort.
//
//   out[c][pixel]  = sum_k f[g_k][c] alpha_k T_k          over the list positions k < n_contrib[pixel]      (no background term)
//   dL/df[g][c]    = sum_pixels sum_{k: g_k = g} alpha_k T_k dL/dout[c][pixel]
//
// The geometry is CONSTANT in this file's kernels: alpha and T come from the saved records, and neither kernel sends a gradient to means,
// scales, rotations or opacities (that gradient is render_aux_bwd.hip's, a back-to-front replay).  That is also why the adjoint needs no
// back-to-front replay: w = alpha T depends only on what lies in front, so both kernels take the same front-to-back walk.
//
// The walk — tile, quadrant and pixel, the staged batches, the cull, the early-outs — is render_lists.h's; a kernel here is its per-pair body.
//
// Few tiles with long lists (the DAS3R training shape: 416 tiles of ~11 k entries) leave one workgroup per tile at 1.6 waves per SIMD, so
// both kernels have a second form for them (aux_long_lists: the rule of kernel_choice.h quad_lanes, on the instance count):
//   forward  SPLIT: four workgroups per tile, one per quadrant; the four waves of a workgroup share its 64 pixels and take a quarter of
//            every staged batch each, starting from T = 1; the blend is a composition of segments — (T, sum) o (T', sum') =
//            (T T', sum + T sum') — so the waves meet once per batch in LDS (four transmittances per pixel, multiplied in wave order)
//            and once at the end (four sums, added in wave order).  No scratch, no atomics, the same bits from run to run.
//   adjoint  bucket-parallel: gridDim.y workgroups per tile, each on the BUCKETs (common.h) of the list it owns, a pixel's T at a bucket
//            start read from the checkpoint the forward left there (render_common.h ckpt_slot: every forward kernel writes them).
//            The buckets' rows are disjoint: nothing meets.
//
// Adjoint: the 64 pixels of a wave are reduced on the cross-lane network (a fixed tree), every wave STORES its sum into its own LDS
// column (an entry is visited at most once per wave and batch), the four columns are added in the order 0, 1, 2, 3 and the row goes
// to partial[emission slot][C]; aux_gather_kernel then adds a Gaussian's consecutive rows in index order.  No floating-point atomics,
// no unordered LDS adds: bit-identical from run to run.
#include "render_lists.h"
#include <algorithm>

namespace das3r {

template <int C, bool SPLIT>
__global__ void __launch_bounds__(256) render_aux_forward_kernel(const ListArgs a, const float *__restrict__ feat /*[P,C]*/, float *__restrict__ out /*[C,H,W]*/,
                                                                 int tile_blocks /*SPLIT: xcd_grid, the blocks of one quadrant*/) {
    __shared__ float4 s_xyh[TILE_PIX], s_co[TILE_PIX];
    __shared__ float s_f[TILE_PIX * C];   // row j = the feature row of staged entry j (wave-uniform reads: broadcasts)
    __shared__ float s_T[SPLIT ? 4 * WAVE : 1];   // SPLIT: every wave's transmittance over its quarter of the batch, per pixel

    // SPLIT: block b is quadrant b / tile_blocks of the tile of block b % tile_blocks (the four on one XCD: tile_blocks is a multiple of 8);
    // the four waves' max_contrib are then equal
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const TileLane t = tile_lane(a, SPLIT ? (int)(blockIdx.x % (unsigned)tile_blocks) : (int)blockIdx.x, SPLIT ? (int)(blockIdx.x / (unsigned)tile_blocks) : wave);
    if (t.tile < 0) return;
    const size_t plane = (size_t)a.H * a.W;
    const auto features = [&](const int j, const uint32_t g) {
#pragma unroll
        for (int c = 0; c < C; c++) s_f[j * C + c] = feat[(size_t)g * C + c];
    };

    float T = 1.0f, acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 0.f;

    if constexpr (SPLIT) {
        const int rounds = ((int)t.max_contrib + TILE_PIX - 1) / TILE_PIX;
        for (int i = 0; i < rounds; i++) {
            const int done_before = i * TILE_PIX;
            const int n = min(TILE_PIX, (int)t.max_contrib - done_before);
            if (i > 0) __syncthreads();   // the previous batch (and its s_T) has been read by every wave
            stage_batch<false>(a, t.range.x + (uint32_t)done_before, n, s_xyh, s_co, nullptr, features);
            __syncthreads();
            // this wave's quarter of the batch, blended from T = 1: (Tseg, seg[]) — then composed with the quarters in front of it
            float Tseg = 1.0f, seg[C];
#pragma unroll
            for (int c = 0; c < C; c++) seg[c] = 0.f;
            // (its own loop over the one mask, on the per-lane copy of the wave's last position: on the shared walk's loop and the scalar
            // t.wmax this kernel, alone of the five, came out 2 - 4 % slower on the training shape — docs/ledger.md (cs))
            const int s = wave * WAVE + lane;
            uint64_t m = __ballot(s < n && quadrant_hit(s_xyh[s], t.qcx, t.qcy));
            while (m != 0ull) {
                const int j = wave * WAVE + __builtin_ctzll(m);
                m &= m - 1ull;
                const uint32_t position = (uint32_t)(done_before + j);
                if (position >= t.wmax_lanes) break;
                const float4 p = s_xyh[j];
                const float4 co = s_co[j];
                float dx, dy, G, alpha;
                const bool active = pair_alpha(p.x, p.y, co, t.pxf, t.pyf, dx, dy, G, alpha) & (position < t.last_contributor);
                if (__ballot(active) == 0ull) continue;
                const float al = active ? alpha : 0.f;
                const float wT = al * Tseg;
#pragma unroll
                for (int c = 0; c < C; c++) seg[c] = __fmaf_rn(s_f[j * C + c], wT, seg[c]);
                Tseg = Tseg * (1.0f - al);
            }
            s_T[wave * WAVE + lane] = Tseg;
            __syncthreads();
            float Tstart = T;   // T in front of this wave's quarter: the batch's start times the quarters of the waves before it, in wave order
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const float Tw = s_T[w * WAVE + lane];
                Tstart = w < wave ? Tstart * Tw : Tstart;
                T = T * Tw;
            }
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = __fmaf_rn(Tstart, seg[c], acc[c]);
        }
        // the four waves' sums of the same 64 pixels, added in wave order (s_f is free: 4 x 64 x C floats)
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C; c++) s_f[(wave * C + c) * WAVE + lane] = acc[c];
        __syncthreads();
        if (wave == 0 && t.inside) {
#pragma unroll
            for (int c = 0; c < C; c++)
                out[(size_t)c * plane + t.pix] = ((s_f[c * WAVE + lane] + s_f[(C + c) * WAVE + lane]) + s_f[(2 * C + c) * WAVE + lane]) + s_f[(3 * C + c) * WAVE + lane];
        }
    } else {
        walk_list_front_to_back(a, t, s_xyh, s_co, features, [&](const int j, uint32_t, const bool active, const float alpha, float, float, float) {
            const float al = active ? alpha : 0.f;
            const float wT = al * T;
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] = __fmaf_rn(s_f[j * C + c], wT, acc[c]);
            T = T * (1.0f - al);
        });
        if (t.inside) {
#pragma unroll
            for (int c = 0; c < C; c++) out[(size_t)c * plane + t.pix] = acc[c];
        }
    }
}

// C values per lane -> their wave totals: one DPP chain for a single value (the total in lane 63), the transposed reduction of
// render_common.h for more (value q in the lanes with lane >> 3 == q).  writer / widx: which total this lane holds.
template <int C>
__device__ __forceinline__ float aux_reduce(const float v[C], const int lane) {
    if constexpr (C == 1) {
        return wave_sum_to_lane63(v[0]);
    } else {
        float v8[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v8[q] = q < C ? v[q] : 0.f;
        return wave_reduce8_transposed(v8, lane);
    }
}

template <int C>
__global__ void __launch_bounds__(256) render_aux_adjoint_kernel(const ListArgs a, const float *__restrict__ dL_dout /*[C,H,W]*/, float *__restrict__ partial /*[capacity,C]*/,
                                                                 const float4 *__restrict__ ckpt /*the forward's checkpoints of long lists; read when gridDim.y > 1*/) {
    __shared__ float4 s_xyh[TILE_PIX], s_co[TILE_PIX];
    __shared__ uint32_t s_slot[TILE_PIX];      // emission slot of every staged entry = its row of `partial`
    __shared__ float col[4][TILE_PIX * C];     // col[wave][j * C + c]: the wave's sum for staged entry j, channel c

    const int tid = threadIdx.x, lane = __lane_id(), wave = tid >> 6;
    const TileLane t = tile_lane(a, blockIdx.x, wave);
    if (t.tile < 0) return;
    const size_t plane = (size_t)a.H * a.W;
    float g[C];
#pragma unroll
    for (int c = 0; c < C; c++) g[c] = t.inside ? dL_dout[(size_t)c * plane + t.pix] : 0.f;

    // which total this lane holds after aux_reduce
    const bool writer = C == 1 ? lane == 63 : ((lane & 7) == 0 && (lane >> 3) < C);
    const int widx = C == 1 ? 0 : (lane >> 3);
    // bucket-parallel launch (gridDim.y > 1): this workgroup takes the buckets blockIdx.y, + gridDim.y, .. of the tile's list — [lo, hi) each
    const int slices = (int)gridDim.y;
    const int nbuckets = slices > 1 ? max(ckpt_buckets(t.range), 1) : 1;
    const int cpix = (t.py - t.by * TILE_Y) * TILE_X + (t.px - t.bx * TILE_X);   // the pixel's place in a checkpoint slot

    for (int bk = (int)blockIdx.y; bk < nbuckets; bk += slices) {
        const uint32_t lo = slices > 1 ? (uint32_t)bk * BUCKET : 0u;
        const uint32_t hi = slices > 1 ? min(t.len, lo + BUCKET) : t.len;
        const uint32_t max_contrib = t.max_contrib > lo ? min(t.max_contrib, hi) - lo : 0u;   // entries of the bucket some pixel reaches (its first ones)
        const int rounds = ((int)max_contrib + TILE_PIX - 1) / TILE_PIX;

        zero_unreached_rows<C>(a, partial, t.range.x + lo + max_contrib, hi - lo - max_contrib);
        if (max_contrib == 0u) continue;   // (uniform)

        // T in front of the bucket: the forward's own, from its checkpoint (a pixel outside the image has none and blends nothing)
        float T = (bk > 0 && t.inside) ? ckpt_slot(const_cast<float4 *>(ckpt), t.range, t.tile, bk - 1)[cpix].x : 1.0f;
        for (int i = 0; i < rounds; i++) {
            const int done_before = i * TILE_PIX;
            const int n = min(TILE_PIX, (int)max_contrib - done_before);
            stage_batch<false>(a, t.range.x + lo + (uint32_t)done_before, n, s_xyh, s_co, s_slot, NoPayload());
            // every wave zeroes its own column: an entry the wave does not visit (culled, past its pixels' stops) contributes exactly 0
            for (int f = lane; f < TILE_PIX * C; f += WAVE) col[wave][f] = 0.f;
            __syncthreads();

            walk_front_to_back(t, s_xyh, s_co, n, lo + (uint32_t)done_before, [&](const int j, uint32_t, const bool active, const float alpha, float, float, float) {
                const float al = active ? alpha : 0.f;
                const float wT = al * T;
                T = T * (1.0f - al);
                float v[C];
#pragma unroll
                for (int c = 0; c < C; c++) v[c] = wT * g[c];
                const float r = aux_reduce<C>(v, lane);
                if (writer) col[wave][j * C + widx] = r;   // a plain store: (wave, entry) pairs are visited once
            });
            __syncthreads();
            // the four waves' sums in a fixed order -> the row of the entry's emission slot
            for (int f = tid; f < n * C; f += TILE_PIX) {
                const int j = f / C, q = f - j * C;
                partial[(size_t)s_slot[j] * C + q] = ((col[0][f] + col[1][f]) + col[2][f]) + col[3][f];
            }
            __syncthreads();
        }
    }
}

// dL_dfeat[i][c] (= or +=) the rows off_by_gid[i] .. + tiles_touched[i] of `partial`, added in index order; zeros for a Gaussian without
// instances: the output is fully written (das3r_raster_grads' contract).  One thread per (Gaussian, channel): a row is read by C
// neighbouring lanes.
__global__ void __launch_bounds__(256) aux_gather_kernel(int P, int C, const uint32_t *__restrict__ tiles_touched, const uint32_t *__restrict__ off_by_gid,
                                                         const float *__restrict__ partial, float *__restrict__ dL_dfeat, int accumulate, uint32_t cap) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)P * C) return;
    const int i = (int)(idx / C), c = (int)(idx - (int64_t)i * C);
    const uint32_t n = tiles_touched[i];
    float s = 0.f;
    if (n > 0u) {
        const uint32_t e0 = min(off_by_gid[i], cap), e1 = min(e0 + min(n, cap), cap);   // (kept inside the scratch whatever a failed binning left)
        for (uint32_t e = e0; e < e1; e++) s += partial[(size_t)e * C + c];
    }
    dL_dfeat[idx] = accumulate ? dL_dfeat[idx] + s : s;
}

#define AUX_DISPATCH(C, WHAT)                           \
    switch (C) {                                        \
    case 1: { constexpr int CC = 1; WHAT; break; }      \
    case 2: { constexpr int CC = 2; WHAT; break; }      \
    case 3: { constexpr int CC = 3; WHAT; break; }      \
    case 4: { constexpr int CC = 4; WHAT; break; }      \
    case 5: { constexpr int CC = 5; WHAT; break; }      \
    case 6: { constexpr int CC = 6; WHAT; break; }      \
    case 7: { constexpr int CC = 7; WHAT; break; }      \
    default: { constexpr int CC = 8; WHAT; break; }     \
    }

// few tiles, long lists (kernel_choice.h quad_lanes' shapes; from the instance COUNT: the same scene takes the same kernels however
// its buffer was sized): the forward with four workgroups per tile, the adjoint bucket-parallel
static bool aux_long_lists(const Layout &L, int64_t num_rendered) { return L.ntiles <= 1024 && num_rendered >= (int64_t)1024 * L.ntiles; }

int launch_render_aux_forward(int P, int W, int H, int C, const float *feat, float *out, const Buffers &v, int64_t num_rendered, bool debug, hipStream_t s) {
    const int blocks = xcd_grid(v.L);
    const ListArgs lists = list_args(v, W, H, P);
    if (aux_long_lists(v.L, num_rendered)) {
        AUX_DISPATCH(C, DAS3R_LAUNCH((render_aux_forward_kernel<CC, true>), dim3(4 * blocks), dim3(TILE_PIX), 0, s, lists, feat, out, blocks));
    } else {
        AUX_DISPATCH(C, DAS3R_LAUNCH((render_aux_forward_kernel<CC, false>), dim3(blocks), dim3(TILE_PIX), 0, s, lists, feat, out, blocks));
    }
    KERNEL_CHECK(s, debug, "render_aux_forward");
    return DAS3R_OK;
}

int launch_render_aux_adjoint(int P, int W, int H, int C, const float *dL_dout, float *dL_dfeat, int accumulate, float *partial, const Buffers &v, int64_t num_rendered, bool debug, hipStream_t s) {
    // slices = buckets of an average list, as the bucket-parallel backward sizes its grid (render_bwd.hip); a longer list's buckets are taken in turn
    const int slices = aux_long_lists(v.L, num_rendered) ? (int)std::min<int64_t>(32, std::max<int64_t>(1, num_rendered / ((int64_t)BUCKET * std::max(v.L.ntiles, 1)))) : 1;
    AUX_DISPATCH(C, DAS3R_LAUNCH((render_aux_adjoint_kernel<CC>), dim3(xcd_grid(v.L), slices), dim3(TILE_PIX), 0, s, list_args(v, W, H, P),
                                 dL_dout, partial, v.b_ckpt()));
    KERNEL_CHECK(s, debug, "render_aux_adjoint");
    DAS3R_LAUNCH(aux_gather_kernel, dim3(div_up((int64_t)P * C, 256)), dim3(256), 0, s, P, C, v.tiles_touched(),
                 v.g_off_by_gid(), partial, dL_dfeat, accumulate, (uint32_t)v.L.capacity);
    KERNEL_CHECK(s, debug, "aux_gather");
    return DAS3R_OK;
}

// the gather alone, for rows another kernel left (render_aux_bwd.hip: the geometry backward writes them on its own walk)
int launch_aux_gather(int P, int C, const float *partial, float *dL_dfeat, const Buffers &v, bool debug, hipStream_t s) {
    DAS3R_LAUNCH(aux_gather_kernel, dim3(div_up((int64_t)P * C, 256)), dim3(256), 0, s, P, C, v.tiles_touched(),
                 v.g_off_by_gid(), partial, dL_dfeat, 0, (uint32_t)v.L.capacity);
    KERNEL_CHECK(s, debug, "aux_gather");
    return DAS3R_OK;
}

}  // namespace das3r
