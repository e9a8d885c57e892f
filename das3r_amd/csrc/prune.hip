// prune.hip — pruning of transparent Gaussians: selection and stable, out-of-place compaction (include/das3r_raster.h das3r_prune_select /
// das3r_prune_compact; the operation of /root/reference/scene/gaussian_model.py:436-468 prune_points / _prune_optimizer, which the reference
// carries and never calls).  A Gaussian rendered with sigmoid(opacity) * conf below 1/255 is never blended (alpha <= opacity at every pixel) and
// gets no gradient; it still costs every kernel that sweeps P.  The torch form of the operation is some twenty boolean-index kernels with their
// own scans; here one decision pass and ONE pass over up to sixteen tensors.
//
//   prune_flag_kernel   keep flag per Gaussian (parked in dst_index: 0 kept, -1 dropped) + the kept count of each group of 1024 rows
//   prune_scan_kernel   one workgroup: exclusive scan of the group counts in place, the total into count[0]
//   prune_rank_kernel   dst_index[i] = group offset + rank inside the group (ballot / mbcnt per wave, sixteen wave counts through LDS)
//   prune_compact_kernel   lanes over the (row, unit) pairs of every tensor: contiguous loads, stores contiguous in runs of kept rows
//
// Separate launches: nothing is handed from workgroup to workgroup inside one.  The opacity is pretransform_math.h's pre_opacity — the bits the
// rasterizer is given on the fused path — so "dropped at 1/255" means "binned with an empty rectangle" (splat_math.h binned_rect) exactly.
#include <string.h>

#include "common.h"

namespace das3r {

constexpr int PRUNE_THREADS = 256, PRUNE_ITEMS = 4, PRUNE_WAVES = PRUNE_THREADS / WAVE;
static_assert(PRUNE_THREADS * PRUNE_ITEMS == DAS3R_PRUNE_GROUP_ROWS, "group size is part of the ABI (DAS3R_PRUNE_COUNT_WORDS)");
constexpr int SCAN_THREADS = 1024;
constexpr int COMPACT_MAX_TENSORS = 16;
constexpr int COMPACT_ITEMS = 8, COMPACT_CHUNK = 256 * COMPACT_ITEMS;

// max that hands a NaN on, as torch.max does (get_scaling.max(dim=1).values > limit is then false: the row is kept)
__device__ __forceinline__ float nan_max(const float a, const float b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }

__global__ void __launch_bounds__(PRUNE_THREADS) prune_flag_kernel(const int P, const float *__restrict__ opacity_raw, const float *__restrict__ conf_flat,
                                                                   const int64_t *__restrict__ mask_index, const float min_opacity,
                                                                   const float *__restrict__ scaling, const float max_world_scale,
                                                                   const uint8_t *__restrict__ also_drop, int32_t *__restrict__ dst_index,
                                                                   int32_t *__restrict__ group_counts) {
    __shared__ int s_cnt[PRUNE_ITEMS * PRUNE_WAVES];
    const int64_t base = (int64_t)blockIdx.x * DAS3R_PRUNE_GROUP_ROWS;
    const int wave = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < PRUNE_ITEMS; k++) {
        const int64_t i = base + k * PRUNE_THREADS + threadIdx.x;
        bool keep = false;
        if (i < P) {
            const int64_t ci = mask_index != nullptr ? mask_index[i] : i;
            const float eff = pre_opacity(opacity_raw[i], conf_flat[ci]);
            bool drop = eff < min_opacity;   // (NaN: false)
            if (scaling != nullptr && max_world_scale > 0.f) {
                const float m = nan_max(nan_max(pre_scale(scaling[3 * i]), pre_scale(scaling[3 * i + 1])), pre_scale(scaling[3 * i + 2]));
                drop = drop || m > max_world_scale;
            }
            if (also_drop != nullptr) drop = drop || also_drop[i] != 0;
            keep = !drop;
            dst_index[i] = keep ? 0 : -1;
        }
        const unsigned long long b = __ballot(keep);
        if (lane_id() == 0) s_cnt[k * PRUNE_WAVES + wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
#pragma unroll
        for (int j = 0; j < PRUNE_ITEMS * PRUNE_WAVES; j++) n += s_cnt[j];
        group_counts[blockIdx.x] = n;
    }
}

// counts[0 .. n): per-group counts in, their exclusive prefix sums out; *total = their sum.  One workgroup: thread t owns a contiguous run.
__global__ void __launch_bounds__(SCAN_THREADS) prune_scan_kernel(const int n, int32_t *__restrict__ counts, int32_t *__restrict__ total) {
    __shared__ int s_wave[SCAN_THREADS / WAVE];
    const int per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
    int mine = 0;
    for (int j = lo; j < hi; j++) mine += counts[j];
    int incl = mine;   // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int up = __shfl_up(incl, o, WAVE);
        if (lane_id() >= o) incl += up;
    }
    const int wave = threadIdx.x / WAVE;
    if (lane_id() == WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; w++) before += s_wave[w];
    int run = before + incl - mine;
    for (int j = lo; j < hi; j++) {
        const int c = counts[j];
        counts[j] = run;
        run += c;
    }
    if (threadIdx.x == SCAN_THREADS - 1) *total = run;
}

__global__ void __launch_bounds__(PRUNE_THREADS) prune_rank_kernel(const int P, const int32_t *__restrict__ group_offsets, int32_t *__restrict__ dst_index) {
    __shared__ int s_cnt[PRUNE_ITEMS * PRUNE_WAVES];
    const int64_t base = (int64_t)blockIdx.x * DAS3R_PRUNE_GROUP_ROWS;
    const int wave = threadIdx.x / WAVE;
    bool keep[PRUNE_ITEMS];
    int rank[PRUNE_ITEMS];
#pragma unroll
    for (int k = 0; k < PRUNE_ITEMS; k++) {
        const int64_t i = base + k * PRUNE_THREADS + threadIdx.x;
        keep[k] = i < P && dst_index[i] == 0;
        const unsigned long long b = __ballot(keep[k]);
        rank[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));   // kept lanes below this one
        if (lane_id() == 0) s_cnt[k * PRUNE_WAVES + wave] = __popcll(b);
    }
    __syncthreads();
    int off = group_offsets[blockIdx.x];
    int j = 0;
#pragma unroll
    for (int k = 0; k < PRUNE_ITEMS; k++) {
        for (; j < k * PRUNE_WAVES + wave; j++) off += s_cnt[j];   // (row order: item k of wave w comes behind every wave's items below k)
        if (keep[k]) dst_index[base + k * PRUNE_THREADS + threadIdx.x] = off + rank[k];
    }
}

struct CompactTable {
    const char *src[COMPACT_MAX_TENSORS];
    char *dst[COMPACT_MAX_TENSORS];
    uint32_t units_per_row[COMPACT_MAX_TENSORS];
    unsigned long long units[COMPACT_MAX_TENSORS];   // P * units_per_row, below 2^32
    int unit_bytes[COMPACT_MAX_TENSORS];             // 16 | 8 | 4
    int first_chunk[COMPACT_MAX_TENSORS + 1];
    int n;
};

template <typename U>
__device__ __forceinline__ void compact_units(const U *__restrict__ src, U *__restrict__ dst, const uint32_t upr, const unsigned long long units,
                                              const unsigned long long e0, const int32_t *__restrict__ dst_index, const int kept) {
    int32_t d[COMPACT_ITEMS];
    uint32_t col[COMPACT_ITEMS];
    U v[COMPACT_ITEMS];
#pragma unroll
    for (int k = 0; k < COMPACT_ITEMS; k++) {   // the new rows first: every index load is in flight before a payload load waits for one
        const unsigned long long e = e0 + (unsigned long long)(k * 256 + threadIdx.x);
        d[k] = -1;
        col[k] = 0u;
        if (e < units) {
            const uint32_t row = upr == 1u ? (uint32_t)e : (uint32_t)e / upr;
            col[k] = (uint32_t)e - row * upr;
            const int32_t t = dst_index[row];
            d[k] = (t >= 0 && t < kept) ? t : -1;
        }
    }
#pragma unroll
    for (int k = 0; k < COMPACT_ITEMS; k++) {
        v[k] = U();   // (every element defined on both paths: a conditionally written array of 16-byte values is kept in scratch otherwise)
        if (d[k] >= 0) v[k] = src[e0 + (unsigned long long)(k * 256 + threadIdx.x)];
    }
#pragma unroll
    for (int k = 0; k < COMPACT_ITEMS; k++)
        if (d[k] >= 0) dst[(unsigned long long)d[k] * upr + col[k]] = v[k];
}

__global__ void __launch_bounds__(256) prune_compact_kernel(const CompactTable T, const int32_t *__restrict__ dst_index, const int kept) {
    // the tensor this workgroup belongs to, picked with static indices (uniform selects: a dynamic index into the by-value table would go through scratch)
    const char *src = T.src[0];
    char *dst = T.dst[0];
    uint32_t upr = T.units_per_row[0];
    unsigned long long units = T.units[0];
    int ub = T.unit_bytes[0], first = 0;
#pragma unroll
    for (int i = 1; i < COMPACT_MAX_TENSORS; i++)
        if (i < T.n && (int)blockIdx.x >= T.first_chunk[i]) {
            src = T.src[i]; dst = T.dst[i]; upr = T.units_per_row[i]; units = T.units[i]; ub = T.unit_bytes[i]; first = T.first_chunk[i];
        }
    const unsigned long long e0 = (unsigned long long)((int)blockIdx.x - first) * COMPACT_CHUNK;
    if (ub == 16) compact_units<uint4>((const uint4 *)src, (uint4 *)dst, upr, units, e0, dst_index, kept);
    else if (ub == 8) compact_units<uint2>((const uint2 *)src, (uint2 *)dst, upr, units, e0, dst_index, kept);
    else compact_units<uint32_t>((const uint32_t *)src, (uint32_t *)dst, upr, units, e0, dst_index, kept);
}

// the last two steps of a selection for a caller with keep flags of its own (mesh.hip): dst_index holds 0 / -1 per row, group_counts the kept
// rows of every group of DAS3R_PRUNE_GROUP_ROWS
int launch_prune_scan_rank(const int P, int32_t *group_counts, int32_t *total, int32_t *dst_index, hipStream_t s) {
    const int groups = div_up(P, DAS3R_PRUNE_GROUP_ROWS);
    DAS3R_LAUNCH(prune_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, groups, group_counts, total);
    KERNEL_CHECK(s, false, "prune_scan");
    DAS3R_LAUNCH(prune_rank_kernel, dim3(groups), dim3(PRUNE_THREADS), 0, s, P, (const int32_t *)group_counts, dst_index);
    KERNEL_CHECK(s, false, "prune_rank");
    return DAS3R_OK;
}

}  // namespace das3r

using namespace das3r;

extern "C" int das3r_prune_select(int32_t P, const float *opacity_raw, const float *conf_flat, const int64_t *mask_index, float min_opacity,
                                  const float *scaling, float max_world_scale, const uint8_t *also_drop, int32_t *dst_index, int32_t *count,
                                  das3r_stream_t stream) {
    if (P < 0 || !count || (P > 0 && (!opacity_raw || !conf_flat || !dst_index))) {
        set_error("das3r_prune_select: P >= 0, and opacity_raw, conf_flat, dst_index and count are required");
        return DAS3R_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {
        HIP_TRY(hipMemsetAsync(count, 0, sizeof(int32_t), s));
        return DAS3R_OK;
    }
    const int groups = div_up(P, DAS3R_PRUNE_GROUP_ROWS);
    int32_t *group_counts = count + 1;
    DAS3R_LAUNCH(prune_flag_kernel, dim3(groups), dim3(PRUNE_THREADS), 0, s, (int)P, opacity_raw, conf_flat, mask_index, min_opacity, scaling,
                 max_world_scale, also_drop, dst_index, group_counts);
    KERNEL_CHECK(s, false, "prune_flag");
    DAS3R_LAUNCH(prune_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, groups, group_counts, count);
    KERNEL_CHECK(s, false, "prune_scan");
    DAS3R_LAUNCH(prune_rank_kernel, dim3(groups), dim3(PRUNE_THREADS), 0, s, (int)P, (const int32_t *)group_counts, dst_index);
    KERNEL_CHECK(s, false, "prune_rank");
    return DAS3R_OK;
}

extern "C" int das3r_prune_compact(int32_t P, int32_t kept, const int32_t *dst_index, int32_t n, const das3r_prune_tensor *tensors,
                                   das3r_stream_t stream) {
    if (P < 0 || kept < 0 || kept > P || n < 0 || n > COMPACT_MAX_TENSORS || (n > 0 && !tensors) || (P > 0 && !dst_index)) {
        set_error("das3r_prune_compact: 0 <= kept <= P, between 0 and %d tensors per call, dst_index required", COMPACT_MAX_TENSORS);
        return DAS3R_ERR_INVALID_ARG;
    }
    if (P == 0 || kept == 0) return DAS3R_OK;
    CompactTable T;
    memset(&T, 0, sizeof(T));
    long long chunks = 0;
    int k = 0;
    for (int i = 0; i < n; i++) {
        const das3r_prune_tensor &a = tensors[i];
        if (a.row_bytes < 0 || a.row_bytes % 4 != 0 || (a.row_bytes > 0 && (!a.src || !a.dst))) {
            set_error("das3r_prune_compact: bad tensor %d (row_bytes a non-negative multiple of 4, src and dst set)", i);
            return DAS3R_ERR_INVALID_ARG;
        }
        if (a.row_bytes == 0) continue;   // no columns (compact SH moments at degree 0)
        const uintptr_t both = (uintptr_t)a.src | (uintptr_t)a.dst | (uintptr_t)a.row_bytes;
        const int ub = both % 16 == 0 ? 16 : (both % 8 == 0 ? 8 : 4);
        if (both % 4 != 0) { set_error("das3r_prune_compact: tensor %d is not 4-byte aligned", i); return DAS3R_ERR_INVALID_ARG; }
        const unsigned long long upr = (unsigned long long)a.row_bytes / ub, units = (unsigned long long)P * upr;
        if (units >= (1ull << 32)) { set_error("das3r_prune_compact: tensor %d has 2^32 or more units to move", i); return DAS3R_ERR_INVALID_ARG; }
        const char *sb = (const char *)a.src, *se = sb + (size_t)P * a.row_bytes;
        const char *db = (const char *)a.dst, *de = db + (size_t)kept * a.row_bytes;
        if (sb < de && db < se) { set_error("das3r_prune_compact: tensor %d: src and dst overlap (the compaction is out of place)", i); return DAS3R_ERR_INVALID_ARG; }
        T.src[k] = sb; T.dst[k] = (char *)a.dst; T.units_per_row[k] = (uint32_t)upr; T.units[k] = units; T.unit_bytes[k] = ub;
        T.first_chunk[k] = (int)chunks;
        chunks += (long long)((units + COMPACT_CHUNK - 1) / COMPACT_CHUNK);
        k++;
    }
    T.first_chunk[k] = (int)chunks;
    T.n = k;
    if (chunks == 0) return DAS3R_OK;
    if (chunks > 0x7fffffffll) { set_error("das3r_prune_compact: too much to move in one call"); return DAS3R_ERR_INVALID_ARG; }
    hipStream_t s = (hipStream_t)stream;
    DAS3R_LAUNCH(prune_compact_kernel, dim3((unsigned)chunks), dim3(256), 0, s, T, dst_index, (int)kept);
    KERNEL_CHECK(s, false, "prune_compact");
    return DAS3R_OK;
}
