// mesh.hip — clean-up of an extracted triangle mesh: connected components on the device, the selection of the pieces that stay and the remap
// of the faces (include/das3r_raster.h das3r_mesh_components / das3r_mesh_filter_select / das3r_mesh_filter_faces).  Imperfectly masked movers
// and faint floaters leave small closed blobs in a fused TSDF; marching tetrahedra turns each into a piece of mesh.  Everything here is
// integer-valued: two runs are bit-identical and the host twin (das3r_debug_mesh_components_host) gives the kernels' arrays exactly.
//
//   mesh_init_kernel      parent[v] = v, face_count[v] = 0, info = 0
//   mesh_union_kernel     a thread per face: union (a, b) and (b, c) — union-find with MINIMUM roots, parent[v] <= v always
//   mesh_flatten_kernel   a thread per vertex: vertex_label[v] = find(v); the roots counted once per workgroup
//   mesh_face_kernel      a wave per 1024 consecutive faces: face_label, and face_count[root] += the length of every run of equal labels
//   mesh_flag_kernel      keep flag per row (vertex or face: both carry a label) + the kept count of each group of 1024 rows; then prune.hip's
//                         one-workgroup scan and its rank kernel (launch_prune_scan_rank): nothing is handed between workgroups inside a launch
//   mesh_emit_faces_kernel   out_faces[face_dst[f]] = vertex_dst[faces[f]]
//
// The union (Playne & Hawick / Allegretti et al.: hook the larger root under the smaller with an atomic minimum): no thread waits for another
// thread's future action.  mesh_find walks strictly decreasing indices; a union iteration that does not hook (the larger root had stopped being
// one: the atomic returned its newer parent `old` < hi) goes on with the strictly smaller pair (old, lo), which restores the one link the
// minimum may have replaced.  Each loop also carries an iteration cap that can not be reached and sets info[3] if it is.
// Inside the union and flatten launches the parent array is touched ONLY with agent-scope relaxed atomic loads and atomic minima — path halving
// included: a plain store could sit dirty in one XCD's L2 and its write-back overwrite a hook made at the memory side; a minimum never raises
// a word.  After the kernel boundary vertex_label is read with plain loads.
#include <string.h>

#include "common.h"

namespace das3r {

#define MESH_HD __host__ __device__ __forceinline__

constexpr int MESH_THREADS = 256, MESH_WAVES = MESH_THREADS / WAVE;
constexpr int MESH_FACE_ITEMS = 16;                            // chunks of 64 faces a wave walks: one open run is carried from chunk to chunk
constexpr int MESH_FACES_PER_GROUP = MESH_THREADS * MESH_FACE_ITEMS;
constexpr int MESH_FLAG_ITEMS = DAS3R_PRUNE_GROUP_ROWS / MESH_THREADS;
constexpr int32_t MESH_MAX = 1 << 30;                          // vertices / faces per call
constexpr int32_t MESH_GAVE_UP_FIND = 1, MESH_GAVE_UP_UNION = 2, MESH_BAD_PARENT = 4;   // info[3]

MESH_HD int32_t mesh_load(int32_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}

// *p = min(*p, v) -> what *p held
MESH_HD int32_t mesh_min(int32_t *p, const int32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    const int32_t old = *p;
    if (v < old) *p = v;
    return old;
#endif
}

// The root of v, halving the path on the way (v's parent becomes its grandparent: an ancestor, written as a minimum).  Every step moves to a
// strictly smaller index, so Nv steps can not be used up; a parent outside [0, v] is never followed.
MESH_HD int32_t mesh_find(int32_t *parent, int32_t v, const int32_t Nv, int32_t *gave_up) {
    for (int32_t it = 0; it <= Nv; it++) {
        const int32_t p = mesh_load(parent + v);
        if (p == v) return v;
        if ((uint32_t)p > (uint32_t)v) { *gave_up |= MESH_BAD_PARENT; return v; }
        const int32_t g = mesh_load(parent + p);
        if ((uint32_t)g > (uint32_t)p) { *gave_up |= MESH_BAD_PARENT; return v; }
        if (g != p) mesh_min(parent + v, g);
        v = g;
    }
    *gave_up |= MESH_GAVE_UP_FIND;
    return v;
}

MESH_HD void mesh_union(int32_t *parent, int32_t a, int32_t b, const int32_t Nv, int32_t *gave_up) {
    for (int64_t it = 0; it <= 2 * (int64_t)Nv; it++) {   // (hi + lo falls with every iteration that does not hook)
        a = mesh_find(parent, a, Nv, gave_up);
        b = mesh_find(parent, b, Nv, gave_up);
        if (a == b || *gave_up) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = mesh_min(parent + hi, lo);
        if (old == hi) return;   // hi was a root and hangs under lo now
        a = old;                 // hi had been hooked meanwhile (old < hi): its parent is min(old, lo) now, and (old, lo) are still to be joined
        b = lo;
    }
    *gave_up |= MESH_GAVE_UP_UNION;
}

MESH_HD bool mesh_good_face(const int32_t a, const int32_t b, const int32_t c, const int32_t Nv) {
    return (uint32_t)a < (uint32_t)Nv && (uint32_t)b < (uint32_t)Nv && (uint32_t)c < (uint32_t)Nv;
}

MESH_HD void mesh_union_face(int32_t *parent, const int32_t *faces, const int64_t f, const int32_t Nv, int32_t *gave_up) {
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!mesh_good_face(a, b, c, Nv)) return;
    if (a != b) mesh_union(parent, a, b, Nv, gave_up);
    if (b != c) mesh_union(parent, b, c, Nv, gave_up);
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_init_kernel(const int32_t Nv, int32_t *__restrict__ parent, int32_t *__restrict__ face_count,
                                                                 int32_t *__restrict__ info) {
    const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (v < Nv) {
        parent[v] = (int32_t)v;
        face_count[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 4) info[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_union_kernel(const int32_t Nv, const int32_t Nf, const int32_t *__restrict__ faces, int32_t *parent,
                                                                  int32_t *info) {
    const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (f >= Nf) return;
    int32_t gave_up = 0;
    mesh_union_face(parent, faces, f, Nv, &gave_up);
    if (gave_up) atomicOr(info + 3, gave_up);
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_flatten_kernel(const int32_t Nv, int32_t *parent, int32_t *__restrict__ vertex_label, int32_t *info) {
    __shared__ int s_roots[MESH_WAVES];
    const int64_t v = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    bool root = false;
    if (v < Nv) {
        int32_t gave_up = 0;
        const int32_t r = mesh_find(parent, (int32_t)v, Nv, &gave_up);
        vertex_label[v] = r;
        root = r == (int32_t)v;
        if (gave_up) atomicOr(info + 3, gave_up);
    }
    const unsigned long long b = __ballot(root);
    if (lane_id() == 0) s_roots[threadIdx.x / WAVE] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
#pragma unroll
        for (int w = 0; w < MESH_WAVES; w++) n += s_roots[w];
        if (n) atomicAdd(info + 0, n);
    }
}

// one integer atomic per run of equal labels; the first addition to a root's count also counts the component as face-bearing
__device__ __forceinline__ void mesh_add_run(int32_t *face_count, int32_t *info, const int32_t label, const int32_t len) {
    if (label < 0 || len <= 0) return;
    if (atomicAdd(face_count + label, len) == 0) atomicAdd(info + 1, 1);
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_face_kernel(const int32_t Nv, const int32_t Nf, const int32_t *__restrict__ faces,
                                                                 const int32_t *__restrict__ vertex_label, int32_t *__restrict__ face_label,
                                                                 int32_t *face_count, int32_t *info) {
    const int lane = lane_id();
    const int64_t base = ((int64_t)blockIdx.x * MESH_WAVES + threadIdx.x / WAVE) * (WAVE * MESH_FACE_ITEMS);
    int32_t open_label = -2, open_len = 0, bad = 0;   // wave-uniform: the run that reaches the end of the chunks walked so far
    for (int k = 0; k < MESH_FACE_ITEMS; k++) {
        const int64_t f = base + k * WAVE + lane;
        if (base + k * WAVE >= Nf) break;   // (uniform)
        int32_t label = -3;                 // past the end: a run of its own that is never added
        if (f < Nf) {
            const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
            label = mesh_good_face(a, b, c, Nv) ? vertex_label[a] : -1;
            face_label[f] = label;
        }
        bad += __popcll(__ballot(label == -1));
        int32_t prev = __shfl_up(label, 1, WAVE);
        if (lane == 0) prev = open_label;
        const unsigned long long heads = __ballot(label != prev);
        if (heads == 0ull) {
            open_len += WAVE;
            continue;
        }
        const int first = __ffsll((long long)heads) - 1, last = 63 - __clzll((long long)heads);
        if (lane == 0) mesh_add_run(face_count, info, open_label, open_len + first);
        const unsigned long long above = lane == WAVE - 1 ? 0ull : heads >> (lane + 1);
        if (((heads >> lane) & 1ull) && above != 0ull) mesh_add_run(face_count, info, label, __ffsll((long long)above));
        open_label = __shfl(label, last, WAVE);
        open_len = WAVE - last;
    }
    if (lane == 0) {
        mesh_add_run(face_count, info, open_label, open_len);
        if (bad) atomicAdd(info + 2, bad);
    }
}

// a row (vertex or face) stays iff it carries a label and that component has at least t faces; parked in dst (0 kept, -1 dropped)
__global__ void __launch_bounds__(MESH_THREADS) mesh_flag_kernel(const int32_t n, const int32_t Nv, const int32_t *__restrict__ label,
                                                                 const int32_t *__restrict__ face_count, const int32_t t, int32_t *__restrict__ dst,
                                                                 int32_t *__restrict__ group_counts) {
    __shared__ int s_cnt[MESH_FLAG_ITEMS * MESH_WAVES];
    const int64_t base = (int64_t)blockIdx.x * DAS3R_PRUNE_GROUP_ROWS;
#pragma unroll
    for (int k = 0; k < MESH_FLAG_ITEMS; k++) {
        const int64_t i = base + k * MESH_THREADS + threadIdx.x;
        bool keep = false;
        if (i < n) {
            const int32_t l = label[i];
            keep = (uint32_t)l < (uint32_t)Nv && face_count[l] >= t;
            dst[i] = keep ? 0 : -1;
        }
        const unsigned long long b = __ballot(keep);
        if (lane_id() == 0) s_cnt[k * MESH_WAVES + threadIdx.x / WAVE] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < MESH_FLAG_ITEMS * MESH_WAVES; j++) c += s_cnt[j];
        group_counts[blockIdx.x] = c;
    }
}

__global__ void __launch_bounds__(MESH_THREADS) mesh_emit_faces_kernel(const int32_t Nv, const int32_t Nf, const int32_t kept_v, const int32_t kept_f,
                                                                       const int32_t *__restrict__ faces, const int32_t *__restrict__ face_dst,
                                                                       const int32_t *__restrict__ vertex_dst, int32_t *__restrict__ out_faces) {
    const int64_t f = (int64_t)blockIdx.x * MESH_THREADS + threadIdx.x;
    if (f >= Nf) return;
    const int32_t d = face_dst[f];
    if ((uint32_t)d >= (uint32_t)kept_f) return;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int32_t v = faces[3 * f + c];
        const int32_t nv = (uint32_t)v < (uint32_t)Nv ? vertex_dst[v] : -1;
        out_faces[3 * (int64_t)d + c] = (uint32_t)nv < (uint32_t)kept_v ? nv : -1;   // (a kept face's vertices are kept: -1 is never written)
    }
}

static inline int mesh_groups(const int32_t n) { return div_up(n, DAS3R_PRUNE_GROUP_ROWS); }

static int mesh_check_sizes(const char *who, const int32_t Nv, const int32_t Nf) {
    if (Nv < 0 || Nf < 0 || Nv > MESH_MAX || Nf > MESH_MAX) {
        set_error("%s: 0 <= Nv, Nf <= 2^30", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    return DAS3R_OK;
}

}  // namespace das3r

using namespace das3r;

extern "C" size_t das3r_mesh_components_workspace_bytes(int32_t Nv, int32_t Nf) {
    if (Nv < 0 || Nf < 0 || Nv > MESH_MAX || Nf > MESH_MAX) return 0;
    return sizeof(int32_t) * ((size_t)Nv + (size_t)mesh_groups(Nv) + (size_t)mesh_groups(Nf)) + 256;
}

extern "C" int das3r_mesh_components(int32_t Nv, int32_t Nf, const int32_t *faces, int32_t *vertex_label, int32_t *face_label, int32_t *face_count,
                                     int32_t *info, int32_t *info_host, char *workspace, das3r_stream_t stream) {
    const char *who = "das3r_mesh_components";
    if (const int rc = mesh_check_sizes(who, Nv, Nf)) return rc;
    if (!info || !info_host || !workspace || (Nv > 0 && (!vertex_label || !face_count)) || (Nf > 0 && (!faces || !face_label))) {
        set_error("%s: faces, vertex_label, face_label, face_count, info, info_host and the workspace are required", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    if ((uintptr_t)workspace % 4 != 0) { set_error("%s: the workspace must be 4-byte aligned", who); return DAS3R_ERR_INVALID_ARG; }
    hipStream_t s = (hipStream_t)stream;
    int32_t *parent = (int32_t *)workspace;
    DAS3R_LAUNCH(mesh_init_kernel, dim3(Nv > 0 ? div_up(Nv, MESH_THREADS) : 1), dim3(MESH_THREADS), 0, s, Nv, parent, face_count, info);
    KERNEL_CHECK(s, false, "mesh_init");
    if (Nv > 0 && Nf > 0) {
        DAS3R_LAUNCH(mesh_union_kernel, dim3(div_up(Nf, MESH_THREADS)), dim3(MESH_THREADS), 0, s, Nv, Nf, faces, parent, info);
        KERNEL_CHECK(s, false, "mesh_union");
    }
    if (Nv > 0) {
        DAS3R_LAUNCH(mesh_flatten_kernel, dim3(div_up(Nv, MESH_THREADS)), dim3(MESH_THREADS), 0, s, Nv, parent, vertex_label, info);
        KERNEL_CHECK(s, false, "mesh_flatten");
    }
    if (Nf > 0) {
        DAS3R_LAUNCH(mesh_face_kernel, dim3(div_up(Nf, MESH_FACES_PER_GROUP)), dim3(MESH_THREADS), 0, s, Nv, Nf, faces, (const int32_t *)vertex_label,
                     face_label, face_count, info);
        KERNEL_CHECK(s, false, "mesh_face");
    }
    HIP_TRY(hipMemcpyAsync(info_host, info, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (info_host[3] != 0) {
        set_error("%s: a loop gave up (info[3] = %d): this can not happen on a parent array only these kernels write", who, (int)info_host[3]);
        return DAS3R_ERR_OVERFLOW;
    }
    return DAS3R_OK;
}

extern "C" int das3r_mesh_filter_select(int32_t Nv, int32_t Nf, const int32_t *vertex_label, const int32_t *face_label, const int32_t *face_count,
                                        int32_t min_count, int32_t *vertex_dst, int32_t *face_dst, int32_t *totals, int32_t *totals_host,
                                        char *workspace, das3r_stream_t stream) {
    const char *who = "das3r_mesh_filter_select";
    if (const int rc = mesh_check_sizes(who, Nv, Nf)) return rc;
    if (min_count < 1) { set_error("%s: the threshold must be at least 1 (faceless vertices always go)", who); return DAS3R_ERR_INVALID_ARG; }
    if (!totals || !totals_host || !workspace || (Nv > 0 && (!vertex_label || !face_count || !vertex_dst)) || (Nf > 0 && (!face_label || !face_dst))) {
        set_error("%s: vertex_label, face_label, face_count, vertex_dst, face_dst, totals, totals_host and the workspace are required", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    if ((uintptr_t)workspace % 4 != 0) { set_error("%s: the workspace must be 4-byte aligned", who); return DAS3R_ERR_INVALID_ARG; }
    totals_host[0] = totals_host[1] = 0;
    if (Nv == 0 || Nf == 0) {   // no face: nothing stays.  Only the dropped marks are written.
        hipStream_t s = (hipStream_t)stream;
        HIP_TRY(hipMemsetAsync(totals, 0, 2 * sizeof(int32_t), s));
        if (Nv > 0) HIP_TRY(hipMemsetAsync(vertex_dst, 0xff, (size_t)Nv * sizeof(int32_t), s));
        if (Nf > 0) HIP_TRY(hipMemsetAsync(face_dst, 0xff, (size_t)Nf * sizeof(int32_t), s));
        return DAS3R_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    int32_t *groups_v = (int32_t *)workspace + Nv, *groups_f = groups_v + mesh_groups(Nv);   // behind the parent array of das3r_mesh_components
    DAS3R_LAUNCH(mesh_flag_kernel, dim3(mesh_groups(Nv)), dim3(MESH_THREADS), 0, s, Nv, Nv, vertex_label, face_count, min_count, vertex_dst, groups_v);
    KERNEL_CHECK(s, false, "mesh_flag (vertices)");
    DAS3R_LAUNCH(mesh_flag_kernel, dim3(mesh_groups(Nf)), dim3(MESH_THREADS), 0, s, Nf, Nv, face_label, face_count, min_count, face_dst, groups_f);
    KERNEL_CHECK(s, false, "mesh_flag (faces)");
    if (const int rc = launch_prune_scan_rank(Nv, groups_v, totals + 0, vertex_dst, s)) return rc;
    if (const int rc = launch_prune_scan_rank(Nf, groups_f, totals + 1, face_dst, s)) return rc;
    HIP_TRY(hipMemcpyAsync(totals_host, totals, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DAS3R_OK;
}

extern "C" int das3r_mesh_filter_faces(int32_t Nv, int32_t Nf, int32_t kept_vertices, int32_t kept_faces, const int32_t *faces, const int32_t *face_dst,
                                       const int32_t *vertex_dst, int32_t *out_faces, das3r_stream_t stream) {
    const char *who = "das3r_mesh_filter_faces";
    if (const int rc = mesh_check_sizes(who, Nv, Nf)) return rc;
    if (kept_vertices < 0 || kept_vertices > Nv || kept_faces < 0 || kept_faces > Nf) {
        set_error("%s: 0 <= kept_vertices <= Nv and 0 <= kept_faces <= Nf", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    if (kept_faces == 0) return DAS3R_OK;
    if (!faces || !face_dst || !vertex_dst || !out_faces) {
        set_error("%s: faces, face_dst, vertex_dst and out_faces are required", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    DAS3R_LAUNCH(mesh_emit_faces_kernel, dim3(div_up(Nf, MESH_THREADS)), dim3(MESH_THREADS), 0, s, Nv, Nf, kept_vertices, kept_faces, faces, face_dst,
                 vertex_dst, out_faces);
    KERNEL_CHECK(s, false, "mesh_emit_faces");
    return DAS3R_OK;
}

// Test aid, host-only: the kernels' own union and find, serially over HOST memory (no device, no HIP call).  face_count may be NULL.
extern "C" int das3r_debug_mesh_components_host(int32_t Nv, int32_t Nf, const int32_t *faces, int32_t *vertex_label, int32_t *face_label,
                                                int32_t *face_count, int32_t *info) {
    const char *who = "das3r_debug_mesh_components_host";
    if (const int rc = mesh_check_sizes(who, Nv, Nf)) return rc;
    if (!info || (Nv > 0 && (!vertex_label || !face_count)) || (Nf > 0 && (!faces || !face_label))) {
        set_error("%s: faces, vertex_label, face_label, face_count and info are required", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    int32_t *parent = vertex_label;   // flattened in place: serially, find(v) of a later vertex only meets finished ones
    int32_t gave_up = 0;
    info[0] = info[1] = info[2] = info[3] = 0;
    for (int32_t v = 0; v < Nv; v++) {
        parent[v] = v;
        face_count[v] = 0;
    }
    for (int64_t f = 0; f < Nf; f++) mesh_union_face(parent, faces, f, Nv, &gave_up);
    for (int32_t v = 0; v < Nv; v++) {
        const int32_t r = mesh_find(parent, v, Nv, &gave_up);
        parent[v] = r;
        info[0] += r == v;
    }
    for (int64_t f = 0; f < Nf; f++) {
        const int32_t a = faces[3 * f];
        const bool good = mesh_good_face(a, faces[3 * f + 1], faces[3 * f + 2], Nv);
        face_label[f] = good ? vertex_label[a] : -1;
        if (good) info[1] += face_count[vertex_label[a]]++ == 0;
        else info[2]++;
    }
    info[3] = gave_up;
    if (gave_up) { set_error("%s: a loop gave up (info[3] = %d)", who, (int)gave_up); return DAS3R_ERR_OVERFLOW; }
    return DAS3R_OK;
}
