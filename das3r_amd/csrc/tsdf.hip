// tsdf.hip — TSDF fusion of depth images into a dense voxel grid, and a triangle mesh out of the grid by marching tetrahedra
// (include/das3r_raster.h das3r_tsdf_integrate / das3r_tsdf_extract_count / das3r_tsdf_extract_emit; the torch form of the integration is
// das3r_amd/tsdf.py integrate_torch, which fixes the operation order this file mirrors operation for operation).  The last step of the
// 2DGS recipe: the per-view surface depths (render_median.hip) become ONE surface with colours and normals.
//
//   tsdf_integrate_kernel   a thread per voxel, x fastest: the view loop runs inside with T, W and the colour in registers, so a batch of
//                           views costs one read and one write of the grid.  The per-view constants (16 matrix floats from a device array,
//                           the two tangents from the kernel arguments) are wave-uniform.  No atomics, no LDS, nothing waits.
//   tsdf_count_kernel       a thread per voxel: the 7-bit mask of its owned lattice edges that carry a vertex and the triangle count of its
//                           cube, parked in cell[] ; the totals of each group of 256 voxels
//   tsdf_scan_kernel        one workgroup: exclusive scan of both group totals in place, (Nv, Nf) into totals[0..1]
//   tsdf_base_kernel        a thread per voxel: its exclusive vertex and triangle base (group offset + rank inside the group)
//   tsdf_emit_kernel        a thread per voxel: its vertices (position, normal, colour) and its cube's triangles; a triangle finds a vertex
//                           as the owner's base + the popcount of the owner's mask bits below the edge type
//
// Separate launches: nothing is handed from workgroup to workgroup inside one.  Every discrete decision is a comparison of fp32 values that
// plain IEEE arithmetic reproduces (Makefile EXACT: no FMA contraction); which way a triangle winds is a table of integer determinants of
// lattice vectors (tsdf_swap_bits), never a function of interpolated positions.  The per-voxel functions are __host__ __device__: the two
// das3r_debug_tsdf_*_host entries run exactly them on host memory, so the arithmetic is testable without a device.
#include <float.h>
#include <math.h>

#include "common.h"

namespace das3r {

#define TSDF_HD __host__ __device__ __forceinline__

constexpr int TSDF_THREADS = 256;
static_assert(TSDF_THREADS == DAS3R_TSDF_GROUP_VOXELS, "group size is part of the ABI (das3r_tsdf_extract_workspace_bytes)");
constexpr int TSDF_SCAN_THREADS = 1024;
constexpr int TSDF_MAX_IMAGE = 16384;   // pixel coordinates stay exact in fp32 far beyond this; the bound keeps V * H * W index arithmetic honest

TSDF_HD bool tsdf_finite(const float v) { return fabsf(v) <= FLT_MAX; }   // (NaN and the infinities fail)

// ---------------------------------------------------------------------------------------------------------------- integration
struct TsdfGridArgs {
    int nx, ny, nz;
    float ox, oy, oz, e;
    float *tsdf, *weight, *colour;   // colour: [3, nz, ny, nx] or null
};
struct TsdfViewArgs {
    int nv, H, W;
    const float *viewmatrix;   // [nv, 16] in device memory, the rasterizer's layout (row-vector convention: splat_math.h xform43)
    float tanx[DAS3R_TSDF_MAX_VIEWS], tany[DAS3R_TSDF_MAX_VIEWS];
    const float *depth, *colour, *weight;   // [nv, H, W], [nv, 3, H, W] or null, [nv, H, W] or null
    float trunc, near_z;
};

// One view's observation of the voxel centred at (X, Y, Z): integrate_torch's steps 1 - 5, in its order.
TSDF_HD bool tsdf_observe(const float *m, const float tanx, const float tany, const int H, const int W, const float *depth, const float *colour,
                          const float *weight, const float trunc, const float near_z, const float X, const float Y, const float Z, float &T,
                          float &Wt, float &Cr, float &Cg, float &Cb) {
    const float xc = m[0] * X + m[4] * Y + m[8] * Z + m[12];
    const float yc = m[1] * X + m[5] * Y + m[9] * Z + m[13];
    const float zc = m[2] * X + m[6] * Y + m[10] * Z + m[14];
    if (!(zc > near_z)) return false;
    const float u = ((xc / zc) / tanx + 1.f) * (0.5f * (float)W);
    const float v = ((yc / zc) / tany + 1.f) * (0.5f * (float)H);
    if (!(u >= 0.f && u < (float)W && v >= 0.f && v < (float)H)) return false;   // (a NaN fails)
    int px = (int)floorf(u), py = (int)floorf(v);
    px = px < 0 ? 0 : (px > W - 1 ? W - 1 : px);   // (the clamps never act: 0 <= u < W)
    py = py < 0 ? 0 : (py > H - 1 ? H - 1 : py);
    const size_t pix = (size_t)py * W + px;
    const float d = depth[pix];
    if (!(d > 0.f && tsdf_finite(d))) return false;
    const float w = weight != nullptr ? weight[pix] : 1.f;
    if (!(w > 0.f && tsdf_finite(w))) return false;
    const float sdf = d - zc;
    if (sdf < -trunc) return false;
    const float ts = fminf(1.f, sdf / trunc);
    const float Wn = Wt + w;
    T = (T * Wt + ts * w) / Wn;
    if (colour != nullptr) {
        const size_t plane = (size_t)H * W;
        Cr = (Cr * Wt + colour[pix] * w) / Wn;
        Cg = (Cg * Wt + colour[plane + pix] * w) / Wn;
        Cb = (Cb * Wt + colour[2 * plane + pix] * w) / Wn;
    }
    Wt = Wn;
    return true;
}

TSDF_HD void tsdf_integrate_voxel(const TsdfGridArgs &g, const TsdfViewArgs &a, const long long n) {
    const int i = (int)(n % g.nx), j = (int)((n / g.nx) % g.ny), k = (int)(n / ((long long)g.nx * g.ny));
    const float X = g.ox + ((float)i + 0.5f) * g.e, Y = g.oy + ((float)j + 0.5f) * g.e, Z = g.oz + ((float)k + 0.5f) * g.e;
    const size_t nvox = (size_t)g.nx * g.ny * g.nz;
    float T = g.tsdf[n], Wt = g.weight[n], Cr = 0.f, Cg = 0.f, Cb = 0.f;
    bool touched = false;
    if (g.colour != nullptr) { Cr = g.colour[n]; Cg = g.colour[nvox + n]; Cb = g.colour[2 * nvox + n]; }
    const size_t plane = (size_t)a.H * a.W;
    for (int v = 0; v < a.nv; v++)
        touched |= tsdf_observe(a.viewmatrix + 16 * v, a.tanx[v], a.tany[v], a.H, a.W, a.depth + v * plane, a.colour != nullptr ? a.colour + 3 * v * plane : nullptr,
                     a.weight != nullptr ? a.weight + v * plane : nullptr, a.trunc, a.near_z, X, Y, Z, T, Wt, Cr, Cg, Cb);
    if (touched) {   // (a voxel no view has taken is not written at all)
        g.tsdf[n] = T;
        g.weight[n] = Wt;
        if (g.colour != nullptr) { g.colour[n] = Cr; g.colour[nvox + n] = Cg; g.colour[2 * nvox + n] = Cb; }
    }
}

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_integrate_kernel(const TsdfGridArgs g, const TsdfViewArgs a, const long long nvox) {
    const long long n = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (n >= nvox) return;
    tsdf_integrate_voxel(g, a, n);
}

// ---------------------------------------------------------------------------------------------------------------- extraction
// Corners of a cube are 3-bit numbers (bit 0: +x, bit 1: +y, bit 2: +z).  The seven owned edges p -> p + d, in the ABI's order of types.
//   type -> d as a corner: {1, 2, 4, 3, 5, 6, 7} (tsdf_type_corner);  d as a corner -> type: {-, 0, 1, 3, 2, 4, 5, 6} (tsdf_corner_type)
// The six Kuhn tetrahedra 0 -> p1 -> p2 -> 7, the axes added in the order xyz, xzy, yxz, yzx, zxy, zyx
constexpr int TSDF_TET_P1[6] = {1, 1, 2, 2, 4, 4};
constexpr int TSDF_TET_P2[6] = {3, 5, 3, 6, 5, 6};

// The vertex pairs (path positions: the inside-or-not mask `c` has bit q for path position q) of the triangles of case c, in the ABI's order:
// 1 inside (I0O0, I0O1, I0O2); 3 inside (O0I0, O0I1, O0I2); 2 inside (I0O0, I0O1, I1O1), (I0O0, I1O1, I1O0).  -> triangles (0, 1 or 2);
// e[t][k] = {a, b}: the corners of vertex k of triangle t, by path position
struct TsdfCase {
    int n;
    int e[2][3][2];
};
constexpr TsdfCase tsdf_case(const int c) {
    TsdfCase r = {0, {{{0, 0}, {0, 0}, {0, 0}}, {{0, 0}, {0, 0}, {0, 0}}}};
    int I[4] = {0, 0, 0, 0}, O[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int q = 0; q < 4; q++) {
        if ((c >> q) & 1) I[ni++] = q;
        else O[no++] = q;
    }
    if (ni == 1) {
        r.n = 1;
        for (int k = 0; k < 3; k++) { r.e[0][k][0] = I[0]; r.e[0][k][1] = O[k]; }
    } else if (ni == 3) {
        r.n = 1;
        for (int k = 0; k < 3; k++) { r.e[0][k][0] = O[0]; r.e[0][k][1] = I[k]; }
    } else if (ni == 2) {
        r.n = 2;
        r.e[0][0][0] = I[0]; r.e[0][0][1] = O[0];
        r.e[0][1][0] = I[0]; r.e[0][1][1] = O[1];
        r.e[0][2][0] = I[1]; r.e[0][2][1] = O[1];
        r.e[1][0][0] = I[0]; r.e[1][0][1] = O[0];
        r.e[1][1][0] = I[1]; r.e[1][1][1] = O[1];
        r.e[1][2][0] = I[1]; r.e[1][2][1] = O[0];
    }
    return r;
}
// Does the triangle `tri` of (tetrahedron, case) need its last two vertices swapped so that its normal points from the inside corners to the
// outside ones?  Integer arithmetic on lattice vectors: a vertex stands at the sum of its two corners (twice the edge's midpoint; any point
// inside the edge gives the same sign), the direction is |I| * sum(O) - |O| * sum(I).
constexpr bool tsdf_swap(const int tet, const int c, const int tri) {
    const int path[4] = {0, TSDF_TET_P1[tet], TSDF_TET_P2[tet], 7};
    const TsdfCase cs = tsdf_case(c);
    if (tri >= cs.n) return false;
    int P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int k = 0; k < 3; k++)
        for (int ax = 0; ax < 3; ax++) P[k][ax] = ((path[cs.e[tri][k][0]] >> ax) & 1) + ((path[cs.e[tri][k][1]] >> ax) & 1);
    int ni = 0, no = 0, sI[3] = {0, 0, 0}, sO[3] = {0, 0, 0};
    for (int q = 0; q < 4; q++)
        for (int ax = 0; ax < 3; ax++) {
            if ((c >> q) & 1) sI[ax] += (path[q] >> ax) & 1;
            else sO[ax] += (path[q] >> ax) & 1;
        }
    for (int q = 0; q < 4; q++) {
        if ((c >> q) & 1) ni++;
        else no++;
    }
    const int a[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, b[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    const int nrm[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    int dot = 0;
    for (int ax = 0; ax < 3; ax++) dot += nrm[ax] * (ni * sO[ax] - no * sI[ax]);
    return dot < 0;
}
// bit (2 c + tri) of word `tet`
constexpr uint32_t tsdf_swap_bits(const int tet) {
    uint32_t w = 0;
    for (int c = 0; c < 16; c++)
        for (int tri = 0; tri < 2; tri++)
            if (tsdf_swap(tet, c, tri)) w |= 1u << (2 * c + tri);
    return w;
}
constexpr uint32_t TSDF_SWAP[6] = {tsdf_swap_bits(0), tsdf_swap_bits(1), tsdf_swap_bits(2), tsdf_swap_bits(3), tsdf_swap_bits(4), tsdf_swap_bits(5)};
// triangles of a case, and for the emission the six (a, b) pairs of each case packed 2 bits a value: bits [12 t + 4 k + 0..1] = a, [+ 2..3] = b
constexpr uint32_t tsdf_case_bits(const int c) {
    const TsdfCase cs = tsdf_case(c);
    uint32_t w = 0;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 3; k++) w |= (uint32_t)(cs.e[t][k][0] | (cs.e[t][k][1] << 2)) << (12 * t + 4 * k);
    return w | ((uint32_t)cs.n << 24);
}
#define TSDF_C(c) tsdf_case_bits(c)
constexpr uint32_t TSDF_CASE[16] = {TSDF_C(0), TSDF_C(1), TSDF_C(2),  TSDF_C(3),  TSDF_C(4),  TSDF_C(5),  TSDF_C(6),  TSDF_C(7),
                                    TSDF_C(8), TSDF_C(9), TSDF_C(10), TSDF_C(11), TSDF_C(12), TSDF_C(13), TSDF_C(14), TSDF_C(15)};
#undef TSDF_C

struct TsdfField {
    int nx, ny, nz;
    const float *tsdf, *weight, *colour;
};
TSDF_HD bool tsdf_in_grid(const TsdfField &f, const int i, const int j, const int k) {
    return i >= 0 && i < f.nx && j >= 0 && j < f.ny && k >= 0 && k < f.nz;
}
TSDF_HD size_t tsdf_index(const TsdfField &f, const int i, const int j, const int k) { return ((size_t)k * f.ny + j) * f.nx + i; }
// valid: inside the grid, weight > 0 and a finite tsdf; *t: the tsdf of a valid voxel
TSDF_HD bool tsdf_valid(const TsdfField &f, const int i, const int j, const int k, float *t) {
    if (!tsdf_in_grid(f, i, j, k)) return false;
    const size_t n = tsdf_index(f, i, j, k);
    const float v = f.tsdf[n];
    *t = v;
    return f.weight[n] > 0.f && tsdf_finite(v);
}

// The two tables as device code reads them (a constexpr host array cannot be indexed at run time there); the small ones are nibbles of a literal.
__device__ __constant__ uint32_t d_TSDF_SWAP[6] = {TSDF_SWAP[0], TSDF_SWAP[1], TSDF_SWAP[2], TSDF_SWAP[3], TSDF_SWAP[4], TSDF_SWAP[5]};
__device__ __constant__ uint32_t d_TSDF_CASE[16] = {TSDF_CASE[0], TSDF_CASE[1], TSDF_CASE[2],  TSDF_CASE[3],  TSDF_CASE[4],  TSDF_CASE[5],  TSDF_CASE[6],  TSDF_CASE[7],
                                                    TSDF_CASE[8], TSDF_CASE[9], TSDF_CASE[10], TSDF_CASE[11], TSDF_CASE[12], TSDF_CASE[13], TSDF_CASE[14], TSDF_CASE[15]};
TSDF_HD uint32_t tsdf_swap_word(const int tet) {
#ifdef __HIP_DEVICE_COMPILE__
    return d_TSDF_SWAP[tet];
#else
    return TSDF_SWAP[tet];
#endif
}
TSDF_HD uint32_t tsdf_case_word(const int c) {
#ifdef __HIP_DEVICE_COMPILE__
    return d_TSDF_CASE[c];
#else
    return TSDF_CASE[c];
#endif
}
TSDF_HD int tsdf_type_corner(const int type) { return (int)((0x7653421u >> (4 * type)) & 7u); }   // {1, 2, 4, 3, 5, 6, 7}
TSDF_HD int tsdf_corner_type(const int corner) { return (int)((0x65423100u >> (4 * corner)) & 7u); }   // {-, 0, 1, 3, 2, 4, 5, 6}
TSDF_HD int tsdf_tet_p1(const int tet) { return (int)((0x442211u >> (4 * tet)) & 7u); }
TSDF_HD int tsdf_tet_p2(const int tet) { return (int)((0x656353u >> (4 * tet)) & 7u); }
TSDF_HD int tsdf_path_corner(const int tet, const int q) { return q == 0 ? 0 : (q == 1 ? tsdf_tet_p1(tet) : (q == 2 ? tsdf_tet_p2(tet) : 7)); }

// the voxel's cell word: bits 0 - 6 the edge mask, bits 8 - 11 the cube's triangle count
TSDF_HD uint32_t tsdf_count_voxel(const TsdfField &f, const int i, const int j, const int k) {
    uint32_t val = 0, ins = 0;   // bit c: corner c is valid / inside
#pragma unroll
    for (int c = 0; c < 8; c++) {
        float t = 0.f;
        if (tsdf_valid(f, i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1), &t)) {
            val |= 1u << c;
            if (t < 0.f) ins |= 1u << c;
        }
    }
    uint32_t mask = 0;
#pragma unroll
    for (int type = 0; type < 7; type++) {
        const int d = tsdf_type_corner(type);
        if ((val & 1u) && ((val >> d) & 1u) && ((ins & 1u) != ((ins >> d) & 1u))) mask |= 1u << type;
    }
    uint32_t ntri = 0;
    if (val == 0xffu) {
#pragma unroll
        for (int tet = 0; tet < 6; tet++) {
            const uint32_t cnt = (ins & 1u) + ((ins >> tsdf_tet_p1(tet)) & 1u) + ((ins >> tsdf_tet_p2(tet)) & 1u) + ((ins >> 7) & 1u);
            ntri += (cnt == 1u || cnt == 3u) ? 1u : (cnt == 2u ? 2u : 0u);
        }
    }
    return mask | (ntri << 8);
}

// the grid gradient at a voxel, in tsdf units per voxel: per axis the central difference where both neighbours are valid, one-sided where one is, 0 where neither
TSDF_HD void tsdf_gradient(const TsdfField &f, const int i, const int j, const int k, const float t0, float g[3]) {
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        const int di = ax == 0, dj = ax == 1, dk = ax == 2;
        float tp = 0.f, tm = 0.f;
        const bool vp = tsdf_valid(f, i + di, j + dj, k + dk, &tp), vm = tsdf_valid(f, i - di, j - dj, k - dk, &tm);
        g[ax] = (vp && vm) ? (tp - tm) * 0.5f : (vp ? tp - t0 : (vm ? t0 - tm : 0.f));
    }
}

struct TsdfMeshOut {
    float ox, oy, oz, e;
    int Nv, Nf;
    float *vertices, *normals, *colours;
    int32_t *faces;
};

TSDF_HD void tsdf_emit_voxel(const TsdfField &f, const TsdfMeshOut &o, const uint32_t *cell, const int32_t *vbase, const int32_t *fbase, const int i,
                             const int j, const int k) {
    const size_t n = tsdf_index(f, i, j, k), nvox = (size_t)f.nx * f.ny * f.nz;
    const uint32_t word = cell[n], mask = word & 0x7fu, ntri = (word >> 8) & 0xfu;
    if (mask != 0u) {
        const float a = f.tsdf[n];
        float ga[3];
        tsdf_gradient(f, i, j, k, a, ga);
        int at = vbase[n];
        for (int type = 0; type < 7; type++) {
            if (!((mask >> type) & 1u)) continue;
            const int d = tsdf_type_corner(type), dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
            const size_t m = tsdf_index(f, i + dx, j + dy, k + dz);
            const float b = f.tsdf[m];
            float gb[3];
            tsdf_gradient(f, i + dx, j + dy, k + dz, b, gb);
            const float s = a / (a - b);
            if (at >= 0 && at < o.Nv) {
                o.vertices[3 * (size_t)at] = o.ox + (((float)i + 0.5f) + s * (float)dx) * o.e;
                o.vertices[3 * (size_t)at + 1] = o.oy + (((float)j + 0.5f) + s * (float)dy) * o.e;
                o.vertices[3 * (size_t)at + 2] = o.oz + (((float)k + 0.5f) + s * (float)dz) * o.e;
                float nx = ga[0] + s * (gb[0] - ga[0]), ny = ga[1] + s * (gb[1] - ga[1]), nz = ga[2] + s * (gb[2] - ga[2]);
                const float len = sqrtf(nx * nx + ny * ny + nz * nz);
                if (len > 0.f && tsdf_finite(len)) { nx = nx / len; ny = ny / len; nz = nz / len; }
                else { nx = 0.f; ny = 0.f; nz = 0.f; }
                o.normals[3 * (size_t)at] = nx;
                o.normals[3 * (size_t)at + 1] = ny;
                o.normals[3 * (size_t)at + 2] = nz;
                if (o.colours != nullptr) {
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        const float ca = f.colour[ch * nvox + n], cb = f.colour[ch * nvox + m];
                        o.colours[3 * (size_t)at + ch] = ca + s * (cb - ca);
                    }
                }
            }
            at++;
        }
    }
    if (ntri != 0u) {   // (the count pass found all eight corners valid: the cube lies inside the grid)
        uint32_t inside = 0;
#pragma unroll
        for (int c = 0; c < 8; c++)
            if (f.tsdf[tsdf_index(f, i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1))] < 0.f) inside |= 1u << c;
        int at = fbase[n];
        for (int tet = 0; tet < 6; tet++) {
            uint32_t c = 0;
            for (int q = 0; q < 4; q++) c |= ((inside >> tsdf_path_corner(tet, q)) & 1u) << q;
            const uint32_t cw = tsdf_case_word((int)c), sw = tsdf_swap_word(tet);
            const int nt = (int)(cw >> 24);
            for (int t = 0; t < nt; t++) {
                int32_t idx[3];
                for (int v = 0; v < 3; v++) {
                    const uint32_t ab = (cw >> (12 * t + 4 * v)) & 0xfu;
                    const int qa = (int)(ab & 3u), qb = (int)(ab >> 2);
                    const int lo = tsdf_path_corner(tet, qa < qb ? qa : qb), hi = tsdf_path_corner(tet, qa < qb ? qb : qa);   // the owner is the earlier corner of the path
                    const int type = tsdf_corner_type(hi ^ lo);
                    const size_t own = tsdf_index(f, i + (lo & 1), j + ((lo >> 1) & 1), k + ((lo >> 2) & 1));
                    idx[v] = vbase[own] + __builtin_popcount(cell[own] & ((1u << type) - 1u));
                }
                if ((sw >> (2 * c + t)) & 1u) { const int32_t x = idx[1]; idx[1] = idx[2]; idx[2] = x; }
                if (at >= 0 && at < o.Nf) {
                    o.faces[3 * (size_t)at] = idx[0];
                    o.faces[3 * (size_t)at + 1] = idx[1];
                    o.faces[3 * (size_t)at + 2] = idx[2];
                }
                at++;
            }
        }
    }
}

__device__ __forceinline__ void tsdf_ijk(const TsdfField &f, const long long n, int &i, int &j, int &k) {
    i = (int)(n % f.nx);
    j = (int)((n / f.nx) % f.ny);
    k = (int)(n / ((long long)f.nx * f.ny));
}

// inclusive sums over the workgroup's 256 threads of two small integers; s_wave: [2][4] LDS words.  -> exclusive ranks; *tot: the totals
__device__ __forceinline__ void tsdf_block_scan(int a, int b, int *s_wave, int &ea, int &eb, int &ta, int &tb) {
    int ia = a, ib = b;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int ua = __shfl_up(ia, o, WAVE), ub = __shfl_up(ib, o, WAVE);
        if (lane_id() >= o) { ia += ua; ib += ub; }
    }
    const int wave = threadIdx.x / WAVE;
    constexpr int NW = TSDF_THREADS / WAVE;
    if (lane_id() == WAVE - 1) { s_wave[wave] = ia; s_wave[NW + wave] = ib; }
    __syncthreads();
    int ba = 0, bb = 0;
    ta = 0; tb = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        if (w < wave) { ba += s_wave[w]; bb += s_wave[NW + w]; }
        ta += s_wave[w]; tb += s_wave[NW + w];
    }
    ea = ba + ia - a;
    eb = bb + ib - b;
}

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_count_kernel(const TsdfField f, const long long nvox, uint32_t *__restrict__ cell,
                                                                 int32_t *__restrict__ group_v, int32_t *__restrict__ group_f) {
    __shared__ int s_wave[2 * TSDF_THREADS / WAVE];
    const long long n = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
    uint32_t word = 0;
    if (n < nvox) {
        int i, j, k;
        tsdf_ijk(f, n, i, j, k);
        word = tsdf_count_voxel(f, i, j, k);
        cell[n] = word;
    }
    int ea, eb, ta, tb;
    tsdf_block_scan(__builtin_popcount(word & 0x7fu), (int)((word >> 8) & 0xfu), s_wave, ea, eb, ta, tb);
    if (threadIdx.x == 0) { group_v[blockIdx.x] = ta; group_f[blockIdx.x] = tb; }
}

// both arrays of n group totals -> their exclusive prefix sums in place; totals[0] = Nv, totals[1] = Nf.  One workgroup: thread t owns a contiguous run.
__global__ void __launch_bounds__(TSDF_SCAN_THREADS) tsdf_scan_kernel(const int n, int32_t *__restrict__ group_v, int32_t *__restrict__ group_f,
                                                                     int32_t *__restrict__ totals) {
    __shared__ int s_wave[2][TSDF_SCAN_THREADS / WAVE];
    const int per = (n + TSDF_SCAN_THREADS - 1) / TSDF_SCAN_THREADS;
    const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
    int mv = 0, mf = 0;
    for (int q = lo; q < hi; q++) { mv += group_v[q]; mf += group_f[q]; }
    int iv = mv, jf = mf;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int uv = __shfl_up(iv, o, WAVE), uf = __shfl_up(jf, o, WAVE);
        if (lane_id() >= o) { iv += uv; jf += uf; }
    }
    const int wave = threadIdx.x / WAVE;
    if (lane_id() == WAVE - 1) { s_wave[0][wave] = iv; s_wave[1][wave] = jf; }
    __syncthreads();
    int bv = 0, bf = 0;
    for (int w = 0; w < wave; w++) { bv += s_wave[0][w]; bf += s_wave[1][w]; }
    int rv = bv + iv - mv, rf = bf + jf - mf;
    for (int q = lo; q < hi; q++) {
        const int cv = group_v[q], cf = group_f[q];
        group_v[q] = rv; group_f[q] = rf;
        rv += cv; rf += cf;
    }
    if (threadIdx.x == TSDF_SCAN_THREADS - 1) { totals[0] = rv; totals[1] = rf; }
}

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_base_kernel(const long long nvox, const uint32_t *__restrict__ cell, const int32_t *__restrict__ group_v,
                                                                const int32_t *__restrict__ group_f, int32_t *__restrict__ vbase, int32_t *__restrict__ fbase) {
    __shared__ int s_wave[2 * TSDF_THREADS / WAVE];
    const long long n = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
    const uint32_t word = n < nvox ? cell[n] : 0u;
    int ea, eb, ta, tb;
    tsdf_block_scan(__builtin_popcount(word & 0x7fu), (int)((word >> 8) & 0xfu), s_wave, ea, eb, ta, tb);
    if (n < nvox) {
        vbase[n] = group_v[blockIdx.x] + ea;
        fbase[n] = group_f[blockIdx.x] + eb;
    }
}

__global__ void __launch_bounds__(TSDF_THREADS) tsdf_emit_kernel(const TsdfField f, const TsdfMeshOut o, const long long nvox, const uint32_t *__restrict__ cell,
                                                                const int32_t *__restrict__ vbase, const int32_t *__restrict__ fbase) {
    const long long n = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
    if (n >= nvox) return;
    int i, j, k;
    tsdf_ijk(f, n, i, j, k);
    tsdf_emit_voxel(f, o, cell, vbase, fbase, i, j, k);
}

// workspace: cell u32[nvox] | vbase i32[nvox] | fbase i32[nvox] | group_v i32[groups] | group_f i32[groups]
struct TsdfWorkspace {
    uint32_t *cell;
    int32_t *vbase, *fbase, *group_v, *group_f;
    int groups;
};
static TsdfWorkspace tsdf_workspace(char *ws, const long long nvox) {
    TsdfWorkspace w;
    w.groups = (int)((nvox + TSDF_THREADS - 1) / TSDF_THREADS);
    w.cell = (uint32_t *)ws;
    w.vbase = (int32_t *)(w.cell + nvox);
    w.fbase = w.vbase + nvox;
    w.group_v = w.fbase + nvox;
    w.group_f = w.group_v + w.groups;
    return w;
}

// 0, or why the grid is refused
static const char *tsdf_bad_dims(const int32_t *dims, long long *nvox) {
    if (!dims) return "dims is NULL";
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return "every dim must be >= 1";
    const long long n = (long long)dims[0] * dims[1];
    if (n > (long long)DAS3R_TSDF_MAX_VOXELS || n * dims[2] > (long long)DAS3R_TSDF_MAX_VOXELS) return "more than 2^28 voxels";
    *nvox = n * dims[2];
    return nullptr;
}
static bool tsdf_positive_finite(const float v) { return v > 0.f && v <= FLT_MAX; }

static int tsdf_check_integrate(const char *who, const int32_t *dims, const float *origin, float voxel, const float *tsdf, const float *weight,
                                const float *colour, int32_t V, const float *viewmatrix, const float *tanfovx, const float *tanfovy, int32_t H, int32_t W,
                                const float *depth, const float *colour_img, float trunc, float near_z, long long *nvox) {
    if (const char *why = tsdf_bad_dims(dims, nvox)) { set_error("%s: %s", who, why); return DAS3R_ERR_INVALID_ARG; }
    if (!tsdf || !weight || !origin) { set_error("%s: the grid's tsdf, weight and origin are required", who); return DAS3R_ERR_INVALID_ARG; }
    if (V < 0 || H < 1 || W < 1 || H > TSDF_MAX_IMAGE || W > TSDF_MAX_IMAGE) { set_error("%s: V >= 0 and 1 <= H, W <= %d", who, TSDF_MAX_IMAGE); return DAS3R_ERR_INVALID_ARG; }
    if (V > 0 && (!depth || !viewmatrix || !tanfovx || !tanfovy)) { set_error("%s: depth, viewmatrix, tanfovx and tanfovy are required", who); return DAS3R_ERR_INVALID_ARG; }
    if (!tsdf_positive_finite(voxel) || !tsdf_positive_finite(trunc)) {
        set_error("%s: the voxel edge and trunc must be finite and > 0 (got %g, %g)", who, (double)voxel, (double)trunc);
        return DAS3R_ERR_INVALID_ARG;
    }
    if (!tsdf_finite(near_z) || !tsdf_finite(origin[0]) || !tsdf_finite(origin[1]) || !tsdf_finite(origin[2])) {
        set_error("%s: near and the origin must be finite", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    for (int v = 0; v < V; v++)
        if (!tsdf_positive_finite(tanfovx[v]) || !tsdf_positive_finite(tanfovy[v])) {
            set_error("%s: tanfovx / tanfovy of view %d must be finite and > 0 (got %g, %g)", who, v, (double)tanfovx[v], (double)tanfovy[v]);
            return DAS3R_ERR_INVALID_ARG;
        }
    if ((colour != nullptr) != (colour_img != nullptr) && V > 0) {
        set_error("%s: a colour image needs a colour grid and a colour grid needs a colour image", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    return DAS3R_OK;
}

static void tsdf_fill_views(TsdfViewArgs *a, int v0, int nv, int32_t H, int32_t W, const float *viewmatrix, const float *tanfovx, const float *tanfovy,
                            const float *depth, const float *colour_img, const float *weight_img, float trunc, float near_z) {
    const size_t plane = (size_t)H * W;
    a->nv = nv; a->H = H; a->W = W;
    a->viewmatrix = viewmatrix + 16 * (size_t)v0;
    for (int v = 0; v < DAS3R_TSDF_MAX_VIEWS; v++) {
        a->tanx[v] = v < nv ? tanfovx[v0 + v] : 1.f;
        a->tany[v] = v < nv ? tanfovy[v0 + v] : 1.f;
    }
    a->depth = depth + v0 * plane;
    a->colour = colour_img ? colour_img + 3 * v0 * plane : nullptr;
    a->weight = weight_img ? weight_img + v0 * plane : nullptr;
    a->trunc = trunc; a->near_z = near_z;
}

}  // namespace das3r

using namespace das3r;

extern "C" int das3r_tsdf_integrate(const int32_t *dims, const float *origin, float voxel, float *tsdf, float *weight, float *colour, int32_t V,
                                    const float *viewmatrix, const float *tanfovx, const float *tanfovy, int32_t H, int32_t W, const float *depth,
                                    const float *colour_img, const float *weight_img, float trunc, float near_z, das3r_stream_t stream) {
    long long nvox = 0;
    if (const int rc = tsdf_check_integrate("das3r_tsdf_integrate", dims, origin, voxel, tsdf, weight, colour, V, viewmatrix, tanfovx, tanfovy, H, W, depth,
                                            colour_img, trunc, near_z, &nvox))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    const TsdfGridArgs g = {dims[0], dims[1], dims[2], origin[0], origin[1], origin[2], voxel, tsdf, weight, colour};
    const unsigned blocks = (unsigned)((nvox + TSDF_THREADS - 1) / TSDF_THREADS);
    for (int v0 = 0; v0 < V; v0 += DAS3R_TSDF_MAX_VIEWS) {   // chunks continue from what the grid holds: the bits of the one-by-one form
        TsdfViewArgs a;
        tsdf_fill_views(&a, v0, (V - v0 < DAS3R_TSDF_MAX_VIEWS ? V - v0 : DAS3R_TSDF_MAX_VIEWS), H, W, viewmatrix, tanfovx, tanfovy, depth, colour_img, weight_img, trunc, near_z);
        DAS3R_LAUNCH(tsdf_integrate_kernel, dim3(blocks), dim3(TSDF_THREADS), 0, s, g, a, nvox);
        KERNEL_CHECK(s, false, "tsdf_integrate");
    }
    return DAS3R_OK;
}

extern "C" int das3r_debug_tsdf_integrate_host(const int32_t *dims, const float *origin, float voxel, float *tsdf, float *weight, float *colour, int32_t V,
                                               const float *viewmatrix, const float *tanfovx, const float *tanfovy, int32_t H, int32_t W, const float *depth,
                                               const float *colour_img, const float *weight_img, float trunc, float near_z) {
    long long nvox = 0;
    if (const int rc = tsdf_check_integrate("das3r_debug_tsdf_integrate_host", dims, origin, voxel, tsdf, weight, colour, V, viewmatrix, tanfovx, tanfovy, H, W,
                                            depth, colour_img, trunc, near_z, &nvox))
        return rc;
    const TsdfGridArgs g = {dims[0], dims[1], dims[2], origin[0], origin[1], origin[2], voxel, tsdf, weight, colour};
    for (int v0 = 0; v0 < V; v0 += DAS3R_TSDF_MAX_VIEWS) {
        TsdfViewArgs a;
        tsdf_fill_views(&a, v0, (V - v0 < DAS3R_TSDF_MAX_VIEWS ? V - v0 : DAS3R_TSDF_MAX_VIEWS), H, W, viewmatrix, tanfovx, tanfovy, depth, colour_img, weight_img, trunc, near_z);
        for (long long n = 0; n < nvox; n++) tsdf_integrate_voxel(g, a, n);
    }
    return DAS3R_OK;
}

extern "C" size_t das3r_tsdf_extract_workspace_bytes(const int32_t *dims) {
    long long nvox = 0;
    if (tsdf_bad_dims(dims, &nvox)) return 0;
    const long long groups = (nvox + TSDF_THREADS - 1) / TSDF_THREADS;
    return (size_t)(12 * nvox + 8 * groups);
}

static int tsdf_check_extract(const char *who, const int32_t *dims, const float *tsdf, const float *weight, const void *workspace, long long *nvox) {
    if (const char *why = tsdf_bad_dims(dims, nvox)) { set_error("%s: %s", who, why); return DAS3R_ERR_INVALID_ARG; }
    if (!tsdf || !weight || !workspace) { set_error("%s: tsdf, weight and the workspace are required", who); return DAS3R_ERR_INVALID_ARG; }
    if ((uintptr_t)workspace % 4 != 0) { set_error("%s: the workspace must be 4-byte aligned", who); return DAS3R_ERR_INVALID_ARG; }
    return DAS3R_OK;
}

extern "C" int das3r_tsdf_extract_count(const int32_t *dims, const float *tsdf, const float *weight, char *workspace, int32_t *totals,
                                        das3r_stream_t stream) {
    long long nvox = 0;
    if (const int rc = tsdf_check_extract("das3r_tsdf_extract_count", dims, tsdf, weight, workspace, &nvox)) return rc;
    if (!totals) { set_error("das3r_tsdf_extract_count: totals is required"); return DAS3R_ERR_INVALID_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const TsdfWorkspace w = tsdf_workspace(workspace, nvox);
    const TsdfField f = {dims[0], dims[1], dims[2], tsdf, weight, nullptr};
    DAS3R_LAUNCH(tsdf_count_kernel, dim3(w.groups), dim3(TSDF_THREADS), 0, s, f, nvox, w.cell, w.group_v, w.group_f);
    KERNEL_CHECK(s, false, "tsdf_count");
    DAS3R_LAUNCH(tsdf_scan_kernel, dim3(1), dim3(TSDF_SCAN_THREADS), 0, s, w.groups, w.group_v, w.group_f, totals);
    KERNEL_CHECK(s, false, "tsdf_scan");
    DAS3R_LAUNCH(tsdf_base_kernel, dim3(w.groups), dim3(TSDF_THREADS), 0, s, nvox, (const uint32_t *)w.cell, (const int32_t *)w.group_v,
                 (const int32_t *)w.group_f, w.vbase, w.fbase);
    KERNEL_CHECK(s, false, "tsdf_base");
    return DAS3R_OK;
}

extern "C" int das3r_tsdf_extract_emit(const int32_t *dims, const float *origin, float voxel, const float *tsdf, const float *weight, const float *colour,
                                       const char *workspace, int32_t Nv, int32_t Nf, float *vertices, float *normals, float *colours, int32_t *faces,
                                       das3r_stream_t stream) {
    const char *who = "das3r_tsdf_extract_emit";
    long long nvox = 0;
    if (const int rc = tsdf_check_extract(who, dims, tsdf, weight, workspace, &nvox)) return rc;
    if (!origin || !tsdf_positive_finite(voxel)) { set_error("%s: the origin is required and the voxel edge must be finite and > 0", who); return DAS3R_ERR_INVALID_ARG; }
    if (Nv < 0 || Nf < 0 || (Nv > 0 && (!vertices || !normals)) || (Nf > 0 && !faces)) {
        set_error("%s: Nv, Nf >= 0 (the count pass's totals) and vertices, normals and faces to hold them", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    if ((colour != nullptr) != (colours != nullptr) && Nv > 0) {
        set_error("%s: vertex colours need a colour grid and a colour grid needs somewhere to put them", who);
        return DAS3R_ERR_INVALID_ARG;
    }
    if (Nv == 0 && Nf == 0) return DAS3R_OK;   // an empty surface: no launch
    hipStream_t s = (hipStream_t)stream;
    const TsdfWorkspace w = tsdf_workspace(const_cast<char *>(workspace), nvox);
    const TsdfField f = {dims[0], dims[1], dims[2], tsdf, weight, colour};
    const TsdfMeshOut o = {origin[0], origin[1], origin[2], voxel, Nv, Nf, vertices, normals, colours, faces};
    DAS3R_LAUNCH(tsdf_emit_kernel, dim3(w.groups), dim3(TSDF_THREADS), 0, s, f, o, nvox, (const uint32_t *)w.cell, (const int32_t *)w.vbase,
                 (const int32_t *)w.fbase);
    KERNEL_CHECK(s, false, "tsdf_emit");
    return DAS3R_OK;
}

// The extraction's per-voxel functions on host memory.  workspace as das3r_tsdf_extract_workspace_bytes sizes it; the first call (vertices ==
// NULL) counts into totals[0..1], the second emits what the first counted.
extern "C" int das3r_debug_tsdf_extract_host(const int32_t *dims, const float *origin, float voxel, const float *tsdf, const float *weight, const float *colour,
                                             char *workspace, int32_t *totals, float *vertices, float *normals, float *colours, int32_t *faces) {
    const char *who = "das3r_debug_tsdf_extract_host";
    long long nvox = 0;
    if (const int rc = tsdf_check_extract(who, dims, tsdf, weight, workspace, &nvox)) return rc;
    if (!totals || !origin) { set_error("%s: totals and origin are required", who); return DAS3R_ERR_INVALID_ARG; }
    const TsdfWorkspace w = tsdf_workspace(workspace, nvox);
    const TsdfField f = {dims[0], dims[1], dims[2], tsdf, weight, colour};
    if (!vertices) {
        int32_t nv = 0, nf = 0;
        for (long long n = 0; n < nvox; n++) {
            const int i = (int)(n % f.nx), j = (int)((n / f.nx) % f.ny), k = (int)(n / ((long long)f.nx * f.ny));
            const uint32_t word = tsdf_count_voxel(f, i, j, k);
            w.cell[n] = word;
            w.vbase[n] = nv;
            w.fbase[n] = nf;
            nv += __builtin_popcount(word & 0x7fu);
            nf += (int32_t)((word >> 8) & 0xfu);
        }
        totals[0] = nv;
        totals[1] = nf;
        return DAS3R_OK;
    }
    if (!normals || !faces || (colour != nullptr) != (colours != nullptr)) { set_error("%s: normals, faces and (with a colour grid) colours are required", who); return DAS3R_ERR_INVALID_ARG; }
    const TsdfMeshOut o = {origin[0], origin[1], origin[2], voxel, totals[0], totals[1], vertices, normals, colours, faces};
    for (long long n = 0; n < nvox; n++) {
        const int i = (int)(n % f.nx), j = (int)((n / f.nx) % f.ny), k = (int)(n / ((long long)f.nx * f.ny));
        tsdf_emit_voxel(f, o, w.cell, w.vbase, w.fbase, i, j, k);
    }
    return DAS3R_OK;
}

// the winding table: word `tet` has bit (2 case + triangle) set where that triangle's last two vertices are swapped
extern "C" void das3r_debug_tsdf_swap_table(uint32_t *out) {
    for (int t = 0; t < 6; t++) out[t] = TSDF_SWAP[t];
}
