// splat_math.h — per-Gaussian device maths shared by the forward and backward preprocess kernels.
// Spec: SURVEY.md Appendix A.1-A.5 / A.8 (upstream:cuda_rasterizer/forward.cu, backward.cu, auxiliary.h).
// Files including this header are compiled with -ffp-contract=off (see Makefile) so every expression below is
// evaluated as written in IEEE fp32.
#pragma once
#include <hip/hip_runtime.h>

namespace das3r {

__device__ constexpr float SH_C0 = 0.28209479177387814f;
__device__ constexpr float SH_C1 = 0.4886025119029199f;
__device__ constexpr float SH_C2_0 = 1.0925484305920792f, SH_C2_1 = -1.0925484305920792f, SH_C2_2 = 0.31539156525252005f,
                           SH_C2_3 = -1.0925484305920792f, SH_C2_4 = 0.5462742152960396f;
__device__ constexpr float SH_C3_0 = -0.5900435899266435f, SH_C3_1 = 2.890611442640554f, SH_C3_2 = -0.4570457994644658f,
                           SH_C3_3 = 0.3731763325901154f, SH_C3_4 = -0.4570457994644658f, SH_C3_5 = 1.445305721320277f,
                           SH_C3_6 = -0.5900435899266435f;

// p_row @ M[:, :3] and p_row @ M for a row-vector-layout 4x4 (element [r][c] at 4r+c)
__device__ __forceinline__ float3 xform43(const float3 p, const float *m) {
    return make_float3(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]);
}
__device__ __forceinline__ float4 xform44(const float3 p, const float *m) {
    return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14], m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
}

// rotation matrix of the quaternion (r,x,y,z) AS GIVEN (no normalisation — DAS3R feeds raw parameters,
// /root/reference/gaussian_renderer/__init__.py:91,108)
__device__ __forceinline__ void quat_to_R(const float4 q, float R[3][3]) {
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - r * z);       R[0][2] = 2.f * (x * z + r * y);
    R[1][0] = 2.f * (x * y + r * z);       R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - r * x);
    R[2][0] = 2.f * (x * z - r * y);       R[2][1] = 2.f * (y * z + r * x);       R[2][2] = 1.f - 2.f * (x * x + y * y);
}

// Sigma = (R S)(R S)^T, upper triangle (00,01,02,11,12,22)
__device__ __forceinline__ void cov3d_from_scale_rot(const float3 scale, const float mod, const float4 q, float *cov) {
    float R[3][3];
    quat_to_R(q, R);
    const float s[3] = {mod * scale.x, mod * scale.y, mod * scale.z};
    float Mm[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) Mm[i][k] = R[i][k] * s[k];
#define SIG(i, j) (Mm[i][0] * Mm[j][0] + Mm[i][1] * Mm[j][1] + Mm[i][2] * Mm[j][2])
    cov[0] = SIG(0, 0); cov[1] = SIG(0, 1); cov[2] = SIG(0, 2); cov[3] = SIG(1, 1); cov[4] = SIG(1, 2); cov[5] = SIG(2, 2);
#undef SIG
}

// EWA: clamp the view-space point to 1.3x the frustum, T = J * Rcw (2x3) with Rcw[i][j] = V[4j+i].
__device__ __forceinline__ void ewa_T(const float3 p_view, const float *V, const float focal_x, const float focal_y,
                                      const float tanfovx, const float tanfovy, float T[2][3], float3 &t, bool &clampx, bool &clampy) {
    t = p_view;
    const float limx = 1.3f * tanfovx, limy = 1.3f * tanfovy;
    const float txtz = t.x / t.z, tytz = t.y / t.z;
    clampx = (txtz < -limx || txtz > limx);
    clampy = (tytz < -limy || tytz > limy);
    t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
    t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
    const float J00 = focal_x / t.z, J02 = -(focal_x * t.x) / (t.z * t.z);
    const float J11 = focal_y / t.z, J12 = -(focal_y * t.y) / (t.z * t.z);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        T[0][j] = J00 * V[4 * j + 0] + 0.f * V[4 * j + 1] + J02 * V[4 * j + 2];
        T[1][j] = 0.f * V[4 * j + 0] + J11 * V[4 * j + 1] + J12 * V[4 * j + 2];
    }
}

// T Sigma T^T before the 0.3 px^2 dilation  ->  (a0, b, c0)
__device__ __forceinline__ void cov2d_undilated(const float T[2][3], const float *c3, float &a0, float &b, float &c0) {
    const float S[3][3] = {{c3[0], c3[1], c3[2]}, {c3[1], c3[3], c3[4]}, {c3[2], c3[4], c3[5]}};
    float TS[2][3];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) TS[i][j] = T[i][0] * S[0][j] + T[i][1] * S[1][j] + T[i][2] * S[2][j];
    a0 = TS[0][0] * T[0][0] + TS[0][1] * T[0][1] + TS[0][2] * T[0][2];
    b = TS[0][0] * T[1][0] + TS[0][1] * T[1][1] + TS[0][2] * T[1][2];
    c0 = TS[1][0] * T[1][0] + TS[1][1] * T[1][1] + TS[1][2] * T[1][2];
}

// cov2D = T Sigma T^T + 0.3 I  ->  (a, b, c)   (sums are left to right: the same bits as adding 0.3 to cov2d_undilated's)
__device__ __forceinline__ void cov2d_from_T(const float T[2][3], const float *c3, float &a, float &b, float &c) {
    float a0, c0;
    cov2d_undilated(T, c3, a0, b, c0);
    a = a0 + 0.3f;
    c = c0 + 0.3f;
}

// Antialiasing (das3r_raster_saved.flags bit 4, upstream's 2D mip filter): a splat is blended with its opacity times
// f = sqrt(max(rho, 2.5e-5)), rho = det0 / det, by how much the 0.3 px^2 dilation spreads it out.  det0 = a0 c0 - b^2 of the
// un-dilated entries, det = a c - b^2 of the dilated ones (a = a0 + 0.3, c = c0 + 0.3).
constexpr float AA_RHO_MIN = 2.5e-5f;
__device__ __forceinline__ float aa_rho(const float a0, const float b, const float c0, const float det) { return (a0 * c0 - b * b) / det; }
__device__ __forceinline__ float aa_factor(const float rho) { return sqrtf(fmaxf(rho, AA_RHO_MIN)); }
// ... backward: g_op = dL/d(o f) summed over the compositing passes, op_in = o, the forward's opacity before the factor.  dL/do = g_op f is the
// caller's; dL/df = g_op o reaches the 2D covariance through rho = f^2 — unless f sat at its clamp: dL/drho = g_op o / (2 f)
__device__ __forceinline__ float aa_opacity_grad_to_rho(const float rho, const float f, const float g_op, const float op_in) {
    float aa_drho = 0.f;
    if (rho > AA_RHO_MIN) aa_drho = g_op * op_in / (2.f * f);
    return aa_drho;
}

// Backward of conic = inverse of the dilated 2D covariance (a, b, c) = (ca, cb, cc): the conic sums (gA, gB, gC) -> dL/d(a, b, c), with
// denom = ca cc - cb^2 and denom2inv = 1 / (denom^2 + 1e-7) [upstream computeCov2DCUDA].  The caller holds all of them and calls this under
// `denom2inv != 0` (the per-Gaussian backward computes dL/dcov3D under the same test).  AA: + dL/drho drho/d(a, b, c), rho = aa_r of the
// undilated entries (ca0, cb, cc0); drho/da = (c0 det - det0 c) / det^2 = (c0 - rho c) / det, and so on.
// ONE definition for preprocess_backward_kernel and focal_grad_kernel: the focal gradient is defined as using the backward's dL/d(a, b, c).
template <bool AA>
__device__ __forceinline__ void conic_grad_to_cov2d(const float gA, const float gB, const float gC, const float ca, const float cb, const float cc,
                                                    const float ca0, const float cc0, const float denom, const float denom2inv, const float aa_r,
                                                    const float aa_drho, float &dL_da, float &dL_db, float &dL_dc) {
    dL_da = denom2inv * (-cc * cc * gA + 2 * cb * cc * gB + (denom - ca * cc) * gC);
    dL_dc = denom2inv * (-ca * ca * gC + 2 * ca * cb * gB + (denom - ca * cc) * gA);
    dL_db = denom2inv * 2 * (cb * cc * gA - (denom + 2 * cb * cb) * gB + ca * cb * gC);
    if constexpr (AA) {
        const float k = aa_drho / denom;
        dL_da += k * (cc0 - aa_r * cc);
        dL_dc += k * (ca0 - aa_r * ca);
        dL_db += k * (-2.f * cb * (1.f - aa_r));
    }
}

// A splat's sums over its per-instance rows, columns Q0 .. Q0 + NQ - 1 of the nine the compositing backward left (colour 0 - 2, mean2D 3 - 4,
// conic 5 - 7, opacity 8): the rows e0 .. e0 + n - 1 of partial[I][9], indexed by emission slot (contiguous per splat), in slot order.
// QUADS && row_exists != null (uniform; render_bwd_stream.hip, experiments build): up to four 48-byte rows per instance, partial[I][4][12], one
// per quadrant of the tile that met the splat, row_exists[I][4] saying which — instance by instance, quadrant by quadrant.
template <int Q0, int NQ, bool QUADS>
__device__ __forceinline__ void sum_instance_rows(const float *partial, const uint8_t *row_exists, const uint32_t e0,
                                                  const uint32_t n, float (&acc)[NQ]) {
    if (QUADS && row_exists) {
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t have = *reinterpret_cast<const uint32_t *>(row_exists + (size_t)(e0 + k) * 4);
#pragma unroll
            for (int w = 0; w < 4; w++) {
                if ((have >> (8 * w)) & 0xffu) {   // the row's columns as the float4 words that hold them (rows are 48 bytes) and column 8 alone
                    const float4 *row = reinterpret_cast<const float4 *>(partial + ((size_t)(e0 + k) * 4 + w) * 12);
                    float v[9];
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        if (Q0 < 4 * b + 4 && Q0 + NQ > 4 * b) {
                            const float4 r = row[b];
                            v[4 * b] = r.x; v[4 * b + 1] = r.y; v[4 * b + 2] = r.z; v[4 * b + 3] = r.w;
                        }
                    }
                    if (Q0 + NQ > 8) v[8] = reinterpret_cast<const float *>(row)[8];
#pragma unroll
                    for (int q = 0; q < NQ; q++) acc[q] += v[Q0 + q];
                }
            }
        }
    } else {
        for (uint32_t k = 0; k < n; k++) {
            const float *row = partial + (size_t)(e0 + k) * 9;
#pragma unroll
            for (int q = 0; q < NQ; q++) acc[q] += row[Q0 + q];
        }
    }
}

// tile rectangle touched by a 2D splat of integer radius r (C truncation toward zero, clamped to the grid)
__device__ __forceinline__ void tile_rect(const float px, const float py, const int r, const int tiles_x, const int tiles_y,
                                          int &rminx, int &rminy, int &rmaxx, int &rmaxy) {
    rminx = min(tiles_x, max(0, (int)((px - r) / TILE_X)));
    rminy = min(tiles_y, max(0, (int)((py - r) / TILE_Y)));
    rmaxx = min(tiles_x, max(0, (int)((px + r + TILE_X - 1) / TILE_X)));
    rmaxy = min(tiles_y, max(0, (int)((py + r + TILE_Y - 1) / TILE_Y)));
}

// Tile rectangle actually binned: the upstream 3-sigma square clipped to the axis-aligned box (half extents hx, hy, already
// padded) outside which alpha = opacity*exp(power) < 1/255 on every pixel centre.  Tiles dropped by the clip can only hold
// pairs upstream would `continue` on, so image and gradients are unchanged; only list lengths / num_rendered shrink.
// tight == false reproduces upstream's lists exactly (used by the bit-exact binning tests).
__device__ __forceinline__ void binned_rect(const float4 xyh, const int r, const int tiles_x, const int tiles_y, const bool tight,
                                            int &rminx, int &rminy, int &rmaxx, int &rmaxy) {
    tile_rect(xyh.x, xyh.y, r, tiles_x, tiles_y, rminx, rminy, rmaxx, rmaxy);
    if (tight) {
        if (xyh.z < 0.f) {  // opacity <= 1/255: never visible
            rmaxx = rminx;
            return;
        }
        // pixel centres are integers: the splat can only matter on the centres ceil(x - hx) .. floor(x + hx) (and likewise in y);
        // an interval that contains no integer touches nothing.  The tile of pixel p is p >> 4.
        const float px0 = ceilf(xyh.x - xyh.z), px1 = floorf(xyh.x + xyh.z);
        const float py0 = ceilf(xyh.y - xyh.w), py1 = floorf(xyh.y + xyh.w);
        if (px1 < px0 || py1 < py0 || px1 < 0.f || py1 < 0.f) {
            rmaxx = rminx;
            return;
        }
        const int tx0 = (int)fmaxf(px0, 0.f) >> 4, ty0 = (int)fmaxf(py0, 0.f) >> 4;
        const int tx1 = ((int)fminf(px1, 1.0e6f) >> 4) + 1, ty1 = ((int)fminf(py1, 1.0e6f) >> 4) + 1;
        rminx = max(rminx, tx0);
        rminy = max(rminy, ty0);
        rmaxx = max(rminx, min(rmaxx, tx1));
        rmaxy = max(rminy, min(rmaxy, ty1));
    }
}

// Load the first n3 = 3*(D+1)^2 floats of a (M,3) SH row into registers.  Rows are 16-byte aligned when
// 3*M is a multiple of 4 (M = 4 or 16): read float4; otherwise scalar.
__device__ __forceinline__ void load_sh_row(const float *__restrict__ row, const int D, const bool vec_ok, float sh[48]) {
    const int n3 = 3 * (D + 1) * (D + 1);
    if (vec_ok) {
        const float4 *r4 = reinterpret_cast<const float4 *>(row);
#pragma unroll
        for (int i = 0; i < 12; i++) {
            if (4 * i < n3) {
                const float4 v = r4[i];
                sh[4 * i] = v.x; sh[4 * i + 1] = v.y; sh[4 * i + 2] = v.z; sh[4 * i + 3] = v.w;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 48; i++)
            if (i < n3) sh[i] = row[i];
    }
}

// SH -> RGB (+0.5, clamp at 0).  Basis as /root/reference/utils/sh_utils.py:74-100.  clamp_bits: bit c = channel c clamped.
__device__ __forceinline__ float3 sh_eval(const int deg, const float sh[48], const float x, const float y, const float z) {
    float out[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
#define SHC(k) sh[(k) * 3 + c]
        float r = SH_C0 * SHC(0);
        if (deg > 0) {
            r = r - SH_C1 * y * SHC(1) + SH_C1 * z * SHC(2) - SH_C1 * x * SHC(3);
            if (deg > 1) {
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
                r = r + SH_C2_0 * xy * SHC(4) + SH_C2_1 * yz * SHC(5) + SH_C2_2 * (2.f * zz - xx - yy) * SHC(6) +
                    SH_C2_3 * xz * SHC(7) + SH_C2_4 * (xx - yy) * SHC(8);
                if (deg > 2) {
                    r = r + SH_C3_0 * y * (3.f * xx - yy) * SHC(9) + SH_C3_1 * xy * z * SHC(10) +
                        SH_C3_2 * y * (4.f * zz - xx - yy) * SHC(11) + SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy) * SHC(12) +
                        SH_C3_4 * x * (4.f * zz - xx - yy) * SHC(13) + SH_C3_5 * z * (xx - yy) * SHC(14) +
                        SH_C3_6 * x * (xx - 3.f * yy) * SHC(15);
                }
            }
        }
#undef SHC
        out[c] = r + 0.5f;
    }
    return make_float3(out[0], out[1], out[2]);
}

// basis functions of the real SH up to degree 3 evaluated at unit direction (x,y,z): rgb_c = sum_k b[k] * sh[k][c]
__device__ __forceinline__ void sh_basis(const int D, const float x, const float y, const float z, float b[16]) {
    b[0] = SH_C0;
    if (D > 0) {
        b[1] = -SH_C1 * y;
        b[2] = SH_C1 * z;
        b[3] = -SH_C1 * x;
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = SH_C2_0 * xy;
            b[5] = SH_C2_1 * yz;
            b[6] = SH_C2_2 * (2.f * zz - xx - yy);
            b[7] = SH_C2_3 * xz;
            b[8] = SH_C2_4 * (xx - yy);
            if (D > 2) {
                b[9] = SH_C3_0 * y * (3.f * xx - yy);
                b[10] = SH_C3_1 * xy * z;
                b[11] = SH_C3_2 * y * (4.f * zz - xx - yy);
                b[12] = SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy);
                b[13] = SH_C3_4 * x * (4.f * zz - xx - yy);
                b[14] = SH_C3_5 * z * (xx - yy);
                b[15] = SH_C3_6 * x * (xx - 3.f * yy);
            }
        }
    }
}

// d(rgb_c)/d(dir) for one channel; sh = that channel's coefficients accessed as SHC(k).  Needs D and the unit direction x, y, z with
// xx, yy, zz, xy, yz, xz in scope.  The forward evaluates it once per splat into the geometry buffer's Jacobian planes (sh_ddir_planes);
// the backward evaluates it itself when the forward did not (preprocess_bwd.hip): the same expressions in the same order, the same bits.
#define SH_DDIR(SHC, dRdx, dRdy, dRdz)                                                                                          \
    do {                                                                                                                        \
        dRdx = 0.f; dRdy = 0.f; dRdz = 0.f;                                                                                     \
        if (D > 0) {                                                                                                            \
            dRdx = -SH_C1 * SHC(3);                                                                                             \
            dRdy = -SH_C1 * SHC(1);                                                                                             \
            dRdz = SH_C1 * SHC(2);                                                                                              \
            if (D > 1) {                                                                                                        \
                dRdx += SH_C2_0 * y * SHC(4) + SH_C2_2 * 2.f * -x * SHC(6) + SH_C2_3 * z * SHC(7) + SH_C2_4 * 2.f * x * SHC(8); \
                dRdy += SH_C2_0 * x * SHC(4) + SH_C2_1 * z * SHC(5) + SH_C2_2 * 2.f * -y * SHC(6) + SH_C2_4 * 2.f * -y * SHC(8); \
                dRdz += SH_C2_1 * y * SHC(5) + SH_C2_2 * 2.f * 2.f * z * SHC(6) + SH_C2_3 * x * SHC(7);                       \
                if (D > 2) {                                                                                                    \
                    dRdx += SH_C3_0 * SHC(9) * 3.f * 2.f * xy + SH_C3_1 * SHC(10) * yz + SH_C3_2 * SHC(11) * -2.f * xy +       \
                            SH_C3_3 * SHC(12) * -3.f * 2.f * xz + SH_C3_4 * SHC(13) * (-3.f * xx + 4.f * zz - yy) +            \
                            SH_C3_5 * SHC(14) * 2.f * xz + SH_C3_6 * SHC(15) * 3.f * (xx - yy);                                \
                    dRdy += SH_C3_0 * SHC(9) * 3.f * (xx - yy) + SH_C3_1 * SHC(10) * xz +                                      \
                            SH_C3_2 * SHC(11) * (-3.f * yy + 4.f * zz - xx) + SH_C3_3 * SHC(12) * -3.f * 2.f * yz +            \
                            SH_C3_4 * SHC(13) * -2.f * xy + SH_C3_5 * SHC(14) * -2.f * yz + SH_C3_6 * SHC(15) * -3.f * 2.f * xy; \
                    dRdz += SH_C3_1 * SHC(10) * xy + SH_C3_2 * SHC(11) * 4.f * 2.f * yz +                                      \
                            SH_C3_3 * SHC(12) * 3.f * (2.f * zz - xx - yy) + SH_C3_4 * SHC(13) * 4.f * 2.f * xz +              \
                            SH_C3_5 * SHC(14) * (xx - yy);                                                                      \
                }                                                                                                               \
            }                                                                                                                   \
        }                                                                                                                       \
    } while (0)

// float4 reads are legal when the row is 16-byte aligned and the padded read stays inside the row
__device__ __forceinline__ bool sh_vec_ok(const float *row, const int D, const int M) {
    const int n3 = 3 * (D + 1) * (D + 1);
    return (((uintptr_t)row & 15) == 0) && (((n3 + 3) & ~3) <= 3 * M);
}

__device__ __forceinline__ float3 sh_regs_to_rgb(const int D, const float sh[48], const float3 p, const float *campos,
                                                 uint8_t &clamp_bits) {
    const float dx = p.x - campos[0], dy = p.y - campos[1], dz = p.z - campos[2];
    const float inv = 1.f / sqrtf(dx * dx + dy * dy + dz * dz);
    const float3 r = sh_eval(D, sh, dx * inv, dy * inv, dz * inv);
    clamp_bits = (uint8_t)((r.x < 0.f ? 1 : 0) | (r.y < 0.f ? 2 : 0) | (r.z < 0.f ? 4 : 0));
    return make_float3(fmaxf(r.x, 0.f), fmaxf(r.y, 0.f), fmaxf(r.z, 0.f));
}

// J[3c + k] = d(rgb_c)/d(dir_k), the colour before its clamp, at the direction sh_regs_to_rgb evaluates it at (SH_DDIR: the backward's
// expressions, bit for bit — preprocess_bwd.hip reads these nine floats instead of the SH row when the forward wrote them).
__device__ __forceinline__ void sh_ddir_regs(const int D, const float sh[48], const float3 p, const float *campos, float J[9]) {
    const float dx = p.x - campos[0], dy = p.y - campos[1], dz = p.z - campos[2];
    const float inv = 1.f / sqrtf(dx * dx + dy * dy + dz * dz);
    const float x = dx * inv, y = dy * inv, z = dz * inv;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
#pragma unroll
    for (int c = 0; c < 3; c++) {
#define SHC_REG(k) sh[(k) * 3 + c]
        SH_DDIR(SHC_REG, J[3 * c], J[3 * c + 1], J[3 * c + 2]);
#undef SHC_REG
    }
}

}  // namespace das3r
