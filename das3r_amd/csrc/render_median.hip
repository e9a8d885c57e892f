// render_median.hip — the median depth and the surface-hit index over the lists a forward has left behind, and the adjoint of the depth
// (include/das3r_raster.h das3r_raster_median_forward / das3r_raster_median_adjoint: the definition is fixed there, word for word).
//
//     hit[pixel] = max { k < n : T_k > tau },     T_0 = 1,  T_{k+1} = T_k (1 - alpha_k),     depth[pixel] = z_hit
//
// over the entries the pixel's colour was blended from — the colour's own entries, order, alpha (pair_alpha) and stop at n_contrib; no
// background term.  T never rises, so the hit is the last entry met with T > tau: the first entry behind which T <= tau, or the last
// contributor of a ray that never gets that opaque.  Not a blend of per-Gaussian channels (render_aux.hip): a selection.
//
// Forward (render_median_forward_kernel): render_lists.h's tile, staging and cull, and a front-to-back walk of this file's own — the shared
// walk's loop with one more exit.  Two running values per pixel, T and the list position of the hit; the hit's Gaussian and its z (the
// record's rgbd.w) are read once per pixel at the end, so nothing is staged beside the walk's own two columns.  THE EARLY-OUT is what a
// median has over an expected value: a wave leaves the walk at the first pair behind which none of its pixels has both T > tau and an entry
// left, and the workgroup stops staging once its four waves have left.  It is kept in this file: the shared walk and its three users
// compile as they did.
//
// Adjoint (render_median_adjoint_kernel): dL_dz[i] = sum of g over the pixels whose hit is Gaussian i — every discrete decision held fixed,
// the hit among them.  One workgroup per tile reads (hit_position, g) of its 256 pixels into LDS and writes one float per list entry of the
// tile to the entry's emission slot in a [capacity] scratch row: in a batch of 256 positions that holds some pixel's hit, thread e adds g
// over the pixels whose hit is entry e, in pixel order 0 .. 255 (a fixed order: no atomics, the same bits from run to run); in every other
// batch a zero.  At most 256 batches of a tile take the summing pass.  A position at or past the tile's list length — the empty marker, or
// garbage — matches no entry.  aux_gather_kernel (render_aux.hip) then folds a Gaussian's consecutive rows into dL_dz [P], fully written.
//
// One workgroup per tile in both kernels, accepted as for the siblings (render_distort.hip).
#include "render_lists.h"

namespace das3r {

constexpr uint32_t NO_HIT = 0xFFFFFFFFu;   // hit_position of an empty pixel

// One staged batch front to back, as render_lists.h walk_front_to_back takes it, on the two running values of the median.  Returns whether
// the wave has more to do behind this batch (wave-uniform): false once no pixel of the wave has both T > tau and an entry left.
__device__ __forceinline__ bool median_walk_batch(const TileLane &t, const float4 *s_xyh, const float4 *s_co, const int n, const uint32_t first,
                                                  const float tau, float &T, uint32_t &hit) {
    if (first >= t.wmax) return false;   // (wave-uniform)
    uint64_t masks[4];
    cull_batch(t, s_xyh, n, true, masks);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint64_t m = masks[k];
        while (m != 0ull) {
            const int j = k * 64 + __builtin_ctzll(m);
            m &= m - 1ull;
            const uint32_t position = first + (uint32_t)j;   // 0-based list position
            if (position >= t.wmax) return false;            // (uniform: the bits come in list order)
            const float4 p = s_xyh[j];
            const float4 co = s_co[j];
            float dx, dy, G, alpha;
            const bool active = pair_alpha(p.x, p.y, co, t.pxf, t.pyf, dx, dy, G, alpha) & (position < t.last_contributor);
            if (__ballot(active) == 0ull) continue;
            hit = (active & (T > tau)) ? position : hit;   // T_k > tau: the last such entry is the hit
            T = T * (1.0f - (active ? alpha : 0.f));
            // the early-out: every pixel of the wave is behind its hit or behind its last contributor
            if (__ballot((T > tau) & (position + 1u < t.last_contributor)) == 0ull) return false;
        }
    }
    return true;
}

__global__ void __launch_bounds__(256) render_median_forward_kernel(const ListArgs a, const float tau, float *__restrict__ depth /*[H,W]*/,
                                                                    int32_t *__restrict__ hit_gaussian /*[H,W] or null*/,
                                                                    uint32_t *__restrict__ hit_position /*[H,W] or null*/) {
    __shared__ float4 s_xyh[TILE_PIX], s_co[TILE_PIX];
    __shared__ uint32_t s_open[4];   // wave w has more to do behind the batch just walked

    const int lane = __lane_id(), wave = threadIdx.x >> 6;
    const TileLane t = tile_lane(a, blockIdx.x, wave);
    if (t.tile < 0) return;

    float T = 1.0f;
    uint32_t hit = NO_HIT;
    bool open = true;   // (wave-uniform)
    const int rounds = ((int)t.max_contrib + TILE_PIX - 1) / TILE_PIX;
    for (int i = 0; i < rounds; i++) {
        const int done_before = i * TILE_PIX;
        const int n = min(TILE_PIX, (int)t.max_contrib - done_before);
        if (i > 0) {
            __syncthreads();   // the previous batch has been read by every wave, and every wave has said whether it goes on
            if ((s_open[0] | s_open[1] | s_open[2] | s_open[3]) == 0u) break;   // (uniform over the workgroup; written again behind the next barrier)
        }
        stage_batch<false>(a, t.range.x + (uint32_t)done_before, n, s_xyh, s_co, nullptr, NoPayload());
        __syncthreads();
        open = open && median_walk_batch(t, s_xyh, s_co, n, (uint32_t)done_before, tau, T, hit);
        if (lane == 0) s_open[wave] = open ? 1u : 0u;
    }
    if (t.inside) {
        // hit < n_contrib <= the list's length; the Gaussian and its depth as stage_batch would read them
        const bool have = hit != NO_HIT;
        const uint32_t g = have ? min(a.point_list[t.range.x + min(hit, t.len - 1u)], a.last_g) : 0u;
        depth[t.pix] = have ? a.rgbd[(size_t)g * SPLAT_REC].w : 0.f;
        if (hit_gaussian != nullptr) hit_gaussian[t.pix] = have ? (int32_t)g : -1;
        if (hit_position != nullptr) hit_position[t.pix] = hit;
    }
}

__global__ void __launch_bounds__(256) render_median_adjoint_kernel(const ListArgs a, const float *__restrict__ dL_ddepth /*[H,W]*/,
                                                                    const uint32_t *__restrict__ hit_position /*[H,W]*/,
                                                                    float *__restrict__ rows /*[capacity]*/) {
    __shared__ uint2 s_hit[TILE_PIX];   // pixel p of the tile: (the list position of its hit, or NO_HIT; the bits of its g)

    const int tid = threadIdx.x;
    const TileLane t = tile_lane(a, blockIdx.x, tid >> 6);
    if (t.tile < 0) return;

    uint32_t hp = t.inside ? hit_position[t.pix] : NO_HIT;
    hp = hp < t.len ? hp : NO_HIT;   // the empty marker, or garbage: no entry of this list
    s_hit[tid] = make_uint2(hp, __float_as_uint(t.inside ? dL_ddepth[t.pix] : 0.f));

    const uint32_t batches = (t.len + (uint32_t)TILE_PIX - 1u) / (uint32_t)TILE_PIX;   // (uniform over the workgroup)
    for (uint32_t b = 0; b < batches; b++) {
        // (a barrier: s_hit is written before the first batch reads it)
        const bool summed = __syncthreads_or(hp != NO_HIT && hp / (uint32_t)TILE_PIX == b) != 0;
        const uint32_t e = b * (uint32_t)TILE_PIX + (uint32_t)tid;
        float s = 0.f;
        if (summed) {
            for (int p = 0; p < TILE_PIX; p++) {   // the pixels in a fixed order (every lane reads the same word: broadcasts)
                const uint2 h = s_hit[p];
                s += h.x == e ? __uint_as_float(h.y) : 0.f;
            }
        }
        if (e < t.len) rows[min(a.slot_list[t.range.x + e], a.cap - 1u)] = s;
    }
}

// render_aux.hip's gather, declared here to be launched with this entry's `accumulate`: dL_dfeat[i][c] (= or +=) the rows of Gaussian i
__global__ void aux_gather_kernel(int P, int C, const uint32_t *__restrict__ tiles_touched, const uint32_t *__restrict__ off_by_gid,
                                  const float *__restrict__ partial, float *__restrict__ dL_dfeat, int accumulate, uint32_t cap);

int launch_render_median_forward(int P, int W, int H, float tau, float *depth, int32_t *hit_gaussian, uint32_t *hit_position, const Buffers &v, bool debug, hipStream_t s) {
    DAS3R_LAUNCH(render_median_forward_kernel, dim3(xcd_grid(v.L)), dim3(TILE_PIX), 0, s, list_args(v, W, H, P), tau, depth,
                 hit_gaussian, hit_position);
    KERNEL_CHECK(s, debug, "render_median_forward");
    return DAS3R_OK;
}

int launch_render_median_adjoint(int P, int W, int H, const float *dL_ddepth, const uint32_t *hit_position, float *dL_dz, int accumulate,
                                 float *rows, const Buffers &v, bool debug, hipStream_t s) {
    DAS3R_LAUNCH(render_median_adjoint_kernel, dim3(xcd_grid(v.L)), dim3(TILE_PIX), 0, s, list_args(v, W, H, P), dL_ddepth,
                 hit_position, rows);
    KERNEL_CHECK(s, debug, "render_median_adjoint");
    DAS3R_LAUNCH(aux_gather_kernel, dim3(div_up((int64_t)P, 256)), dim3(256), 0, s, P, 1, v.tiles_touched(),
                 v.g_off_by_gid(), rows, dL_dz, accumulate, (uint32_t)v.L.capacity);
    KERNEL_CHECK(s, debug, "aux_gather");
    return DAS3R_OK;
}

}  // namespace das3r
