// thin.hip — voxel thinning: among the Gaussians whose centres fall into the same cell of a voxel grid keep the best one and tell it how many
// it stands for (include/das3r_raster.h das3r_thin_voxels; the torch form of the same rule is das3r_amd/thin.py voxel_keep_torch).  DAS3R
// starts with one Gaussian per confident pixel of every frame, so a static surface seen in F frames starts as about F coincident Gaussians:
// this is the decision that removes the F-fold redundancy; the surgery itself is prune.hip's (das3r_prune_select(also_drop) + _compact).
//
// No sort: an open-addressing table of S slots, S the power of two >= 2 P (load factor <= 1/2), three arrays and one per-point word:
//
//   key   u64[S]   the cell, 63 bits; all-ones = empty (no real key has bit 63)
//   best  u64[S]   max over the cell's points of  orderable(score) << 32 | (0xFFFFFFFF - i)   — the highest score, ties to the lower index
//   pop   u32[S]   the cell's population
//   slot  i32[P]   the slot of point i, or -1 for a point that is not placeable
//
//   workspace = 20 S + 4 P bytes: 44 - 84 bytes per point; at the DAVIS shape's 7.37 M points S = 2^24, 49.5 bytes per point (365 MB).
//
//   (memsets)           key = all-ones, best = pop = 0, info = {0, 0}
//   thin_insert_kernel  a thread per point: claim or find the slot (64-bit compare-and-swap, linear probing, at most S probes), 64-bit max
//                       into best, add into pop
//   thin_resolve_kernel a thread per point: keep / count from its slot; the kept count into info[0], one add per wave
//
// Separate launches: nothing is handed from workgroup to workgroup inside one, and no thread waits for another — a thread that loses a
// compare-and-swap has either found its own key or moves on.  Which slot a cell lands in depends on who came first; nothing that is written
// out does (max and add commute), so two runs are bit-identical, whatever the launch geometry and the hash.  Every atomic is a vector
// atomic on ordinary device memory.  Compiled without FMA contraction (Makefile EXACT) although the cell is one multiply and a floor.
#include "common.h"

namespace das3r {

constexpr int THIN_THREADS = 256;
constexpr unsigned long long THIN_EMPTY = ~0ull;
constexpr float THIN_HALF = 1048576.f;   // 2^20: cells lie in [-2^20, 2^20) per axis
constexpr int32_t THIN_MAX_P = 1 << 30;  // S <= 2^31: slots fit the per-point int32

static inline unsigned long long thin_slots(int32_t P) {
    unsigned long long s = 64;
    while (s < 2ull * (unsigned long long)P) s <<= 1;
    return s;
}

// a total order on scores as unsigned integers: NaN (0) < -inf < ... < -0 = +0 < ... < +inf
__device__ __forceinline__ uint32_t thin_orderable(const float s) {
    if (s != s) return 0u;
    uint32_t b = __float_as_uint(s);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ unsigned long long thin_mix(unsigned long long k) {   // (murmur3's finaliser: lattices of cells must not line up in the table)
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

__global__ void __launch_bounds__(THIN_THREADS) thin_insert_kernel(const int P, const float *__restrict__ xyz, const float *__restrict__ score,
                                                                  const float inv_edge, unsigned long long *__restrict__ keys,
                                                                  unsigned long long *__restrict__ best, uint32_t *__restrict__ pop,
                                                                  int32_t *__restrict__ slot_of, const unsigned long long slots,
                                                                  int32_t *__restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * THIN_THREADS + threadIdx.x;
    if (i >= P) return;
    const float px = xyz[3 * i] * inv_edge, py = xyz[3 * i + 1] * inv_edge, pz = xyz[3 * i + 2] * inv_edge;
    const float cx = floorf(px), cy = floorf(py), cz = floorf(pz);
    // (a NaN or an infinity fails the range comparisons by itself; the finiteness test is the rule as written)
    const bool placeable = isfinite(px) && isfinite(py) && isfinite(pz) && cx >= -THIN_HALF && cx < THIN_HALF && cy >= -THIN_HALF &&
                           cy < THIN_HALF && cz >= -THIN_HALF && cz < THIN_HALF;
    int32_t found = -1;
    if (placeable) {
        const unsigned long long key = ((unsigned long long)((int)cx + (1 << 20)) << 42) | ((unsigned long long)((int)cy + (1 << 20)) << 21) |
                                       (unsigned long long)((int)cz + (1 << 20));
        const unsigned long long mask = slots - 1ull;
        unsigned long long s = thin_mix(key) & mask;
        for (unsigned long long n = 0; n < slots; n++) {   // bounded: a full table ends the walk, it does not spin
            const unsigned long long prev = atomicCAS(&keys[s], THIN_EMPTY, key);
            if (prev == THIN_EMPTY || prev == key) { found = (int32_t)s; break; }
            s = (s + 1ull) & mask;
        }
        if (found >= 0) {
            const uint32_t o = score != nullptr ? thin_orderable(score[i]) : 0u;
            atomicMax(&best[found], ((unsigned long long)o << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i));
            atomicAdd(&pop[found], 1u);
        } else {
            atomicOr(&info[1], 1);   // exhausted (cannot happen at S >= 2 P): the point is treated as not placeable
        }
    }
    slot_of[i] = found;
}

__global__ void __launch_bounds__(THIN_THREADS) thin_resolve_kernel(const int P, const unsigned long long *__restrict__ best,
                                                                   const uint32_t *__restrict__ pop, const int32_t *__restrict__ slot_of,
                                                                   uint8_t *__restrict__ keep, int32_t *__restrict__ count, int32_t *__restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * THIN_THREADS + threadIdx.x;
    bool kept = false;
    if (i < P) {
        const int32_t s = slot_of[i];
        int32_t c = 1;
        kept = true;
        if (s >= 0) {
            kept = (0xFFFFFFFFu - (uint32_t)best[s]) == (uint32_t)i;
            c = kept ? (int32_t)pop[s] : 0;
        }
        keep[i] = kept ? 1 : 0;
        count[i] = c;
    }
    const unsigned long long b = __ballot(kept);
    if (lane_id() == 0 && b != 0ull) atomicAdd(&info[0], (int)__popcll(b));
}

}  // namespace das3r

using namespace das3r;

extern "C" size_t das3r_thin_workspace_bytes(int32_t P) {
    if (P <= 0 || P > THIN_MAX_P) return 0;
    return (size_t)(20ull * thin_slots(P) + 4ull * (unsigned long long)P);
}

extern "C" int das3r_thin_voxels(int32_t P, const float *xyz, const float *score, float inv_edge, uint8_t *keep, int32_t *count, int32_t *info,
                                 char *workspace, das3r_stream_t stream) {
    if (P < 0 || P > THIN_MAX_P || !info || (P > 0 && (!xyz || !keep || !count || !workspace))) {
        set_error("das3r_thin_voxels: 0 <= P <= 2^30, and xyz, keep, count, info and workspace are required (score may be NULL)");
        return DAS3R_ERR_INVALID_ARG;
    }
    if (!(inv_edge > 0.f) || !(inv_edge <= 3.402823466e38f)) {   // (NaN fails the first, +inf the second)
        set_error("das3r_thin_voxels: inv_edge must be finite and > 0 (got %g)", (double)inv_edge);
        return DAS3R_ERR_INVALID_ARG;
    }
    if (P > 0 && (uintptr_t)workspace % 8 != 0) {
        set_error("das3r_thin_voxels: the workspace must be 8-byte aligned");
        return DAS3R_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(info, 0, 2 * sizeof(int32_t), s));
    if (P == 0) return DAS3R_OK;
    const unsigned long long S = thin_slots(P);
    unsigned long long *keys = (unsigned long long *)workspace, *best = keys + S;
    uint32_t *pop = (uint32_t *)(best + S);
    int32_t *slot_of = (int32_t *)(pop + S);
    HIP_TRY(hipMemsetAsync(keys, 0xFF, (size_t)(8ull * S), s));
    HIP_TRY(hipMemsetAsync(best, 0, (size_t)(12ull * S), s));
    const int blocks = div_up(P, THIN_THREADS);
    DAS3R_LAUNCH(thin_insert_kernel, dim3(blocks), dim3(THIN_THREADS), 0, s, (int)P, xyz, score, inv_edge, keys, best, pop, slot_of, S, info);
    KERNEL_CHECK(s, false, "thin_insert");
    DAS3R_LAUNCH(thin_resolve_kernel, dim3(blocks), dim3(THIN_THREADS), 0, s, (int)P, (const unsigned long long *)best, (const uint32_t *)pop,
                 (const int32_t *)slot_of, keep, count, info);
    KERNEL_CHECK(s, false, "thin_resolve");
    return DAS3R_OK;
}
