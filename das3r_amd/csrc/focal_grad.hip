// focal_grad.hip — dL/d(log-focal offsets) of a backward pass (das3r_raster_backward_focal, api.hip): one per-Gaussian kernel between the
// compositing backward and the per-Gaussian backward, where depth_fold_kernel sits.
//
// s = (s_x, s_y): the forward at s is the forward with tanfovx e^(-s_x), tanfovy e^(-s_y) and the clip-x / clip-y columns of projmatrix
// scaled by e^(s_x) / e^(s_y).  With every discrete decision held fixed (cull, radius, rectangle, lists, the 1/255 and T < 1e-4 cut-offs, the
// EWA clamp flags; the clamped ray a constant, as upstream treats it for the mean) a splat's pixel mean moves as
// (u - (W - 1) / 2) e^(s_x), its undilated covariance as a0 e^(2 s_x), b e^(s_x + s_y), c0 e^(2 s_y); the SH view direction and 1/z do not move.
// So, per rendered splat, from the row sums the compositing backward left (partial[], the rows off_by_gid[i] .. + tiles_touched[i]):
//   c_x = dL/du (u - (W - 1) / 2) + 2 a0 dL/da + b dL/db        c_y = dL/dv (v - (H - 1) / 2) + 2 c0 dL/dc + b dL/db
// with dL/d(a, b, c) exactly preprocess_backward_kernel's (the antialiasing factor's term included), and dL/ds = sum_i c(i).
// No float atomics: a workgroup adds its 256 lanes in a fixed tree and stores one row; focal_finish_kernel adds the rows in a fixed order.
// Nothing needs pre-zeroing: every word of per_splat, of the workspace rows and of sums is written.
#include <algorithm>

#include "common.h"
#include "splat_math.h"
#include "pretransform_math.h"

namespace das3r {

// 256 values per channel in red[c][..] -> red[c][0], the same tree every time (all 256 threads call it)
__device__ __forceinline__ void focal_tree_sum(float (&red)[2][256]) {
    __syncthreads();
#pragma unroll
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
        }
        __syncthreads();
    }
}

template <bool HAS_COV, bool AA>
__global__ void __launch_bounds__(256) focal_grad_kernel(
    int P, const float *__restrict__ means3D, const float *__restrict__ scales, float scale_modifier, const float *__restrict__ rotations,
    const float *__restrict__ cov3D_precomp, const float *__restrict__ opacities /*AA only, without `pre`*/, const PreXform pre,
    const float *__restrict__ viewmatrix, int W, int H, float tanfovx, float tanfovy, const uint32_t *__restrict__ tiles_touched,
    const uint32_t *__restrict__ off_by_gid, const float4 *__restrict__ xyh /*the splat records: (u, v, ..)*/,
    const float *__restrict__ partial /*[I,9] — or, with row_exists, [I][4][12]*/, const uint8_t *__restrict__ row_exists /*[I][4] or null*/,
    float *__restrict__ per_splat /*[P,2] or null*/, float *__restrict__ block_rows /*[gridDim.x][2]*/) {
    __shared__ float red[2][256];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float c_x = 0.f, c_y = 0.f;
    const uint32_t n = i < P ? tiles_touched[i] : 0u;
    if (n > 0u) {
        // the splat's row sums, columns 3 .. 8 (dL/dmean2D x, y; dL/dconic A, B, C; dL/dopacity), in preprocess_backward_kernel's order
        float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const uint32_t e0 = off_by_gid[i];
        if (row_exists) {   // (uniform) up to four 48-byte rows per instance, one per quadrant of the tile that met the splat
            for (uint32_t k = 0; k < n; k++) {
                const uint8_t *have = row_exists + (size_t)(e0 + k) * 4;
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    if (have[w]) {
                        const float *row = partial + ((size_t)(e0 + k) * 4 + w) * 12;
#pragma unroll
                        for (int q = 0; q < 6; q++) acc[q] += row[3 + q];
                    }
                }
            }
        } else {
            for (uint32_t k = 0; k < n; k++) {
                const float *row = partial + (size_t)(e0 + k) * 9;
#pragma unroll
                for (int q = 0; q < 6; q++) acc[q] += row[3 + q];
            }
        }
        // the forward's inputs again (pretransform_math.h: the same bits), its T and its undilated covariance
        float3 mean;
        float c3[6];
        float op_in = 0.f;
        if (!HAS_COV && pre.xyz != nullptr) {   // (uniform)
            PoseRegs pose;
            load_pose(pre.Rm, pre.tv, pre.Lq, pose);
            mean = pre_mean(pose, pre.xyz[3 * i], pre.xyz[3 * i + 1], pre.xyz[3 * i + 2]);
            const float4 q = pre_rot(pose, reinterpret_cast<const float4 *>(pre.rot)[i]);
            const float3 sc = make_float3(pre_scale(pre.scaling[3 * i]), pre_scale(pre.scaling[3 * i + 1]), pre_scale(pre.scaling[3 * i + 2]));
            cov3d_from_scale_rot(sc, scale_modifier, q, c3);
            if constexpr (AA) op_in = pre_opacity(pre.opacity_raw[i], pre.conf_flat[pre.mask_index ? pre.mask_index[i] : (int64_t)i]);
        } else {
            mean = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
            if constexpr (HAS_COV) {
#pragma unroll
                for (int j = 0; j < 6; j++) c3[j] = cov3D_precomp[6 * (size_t)i + j];
            } else {
                const float3 sc = make_float3(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]);
                cov3d_from_scale_rot(sc, scale_modifier, reinterpret_cast<const float4 *>(rotations)[i], c3);
            }
            if constexpr (AA) op_in = opacities[i];
        }
        float V[16];
#pragma unroll
        for (int j = 0; j < 16; j++) V[j] = viewmatrix[j];
        const float focal_x = W / (2.0f * tanfovx), focal_y = H / (2.0f * tanfovy);
        float T[2][3];
        float3 t;
        bool clampx, clampy;
        ewa_T(xform43(mean, V), V, focal_x, focal_y, tanfovx, tanfovy, T, t, clampx, clampy);
        float a0, b, c0;
        cov2d_undilated(T, c3, a0, b, c0);
        // ---- conic sums -> dL/d(a, b, c): preprocess_backward_kernel's expressions
        const float ca = a0 + 0.3f, cc = c0 + 0.3f;
        const float gA = acc[2], gB = acc[3], gC = acc[4];
        const float denom = ca * cc - b * b;
        float aa_r = 0.f, aa_drho = 0.f;
        if constexpr (AA) {
            aa_r = aa_rho(a0, b, c0, denom);
            const float f = aa_factor(aa_r);
            if (aa_r > AA_RHO_MIN) aa_drho = acc[5] * op_in / (2.f * f);
        }
        float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
        const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
        if (denom2inv != 0.f) {
            dL_da = denom2inv * (-cc * cc * gA + 2 * b * cc * gB + (denom - ca * cc) * gC);
            dL_dc = denom2inv * (-ca * ca * gC + 2 * ca * b * gB + (denom - ca * cc) * gA);
            dL_db = denom2inv * 2 * (b * cc * gA - (denom + 2 * b * b) * gB + ca * b * gC);
            if constexpr (AA) {
                const float k = aa_drho / denom;
                dL_da += k * (c0 - aa_r * cc);
                dL_dc += k * (a0 - aa_r * ca);
                dL_db += k * (-2.f * b * (1.f - aa_r));
            }
        }
        // the row sums hold dL/d(ndc) = dL/d(pixel) W / 2 (the compositing backward's ddelx_dx): dL/du (u - (W - 1) / 2) = acc (that / (W / 2))
        const float4 rec = xyh[(size_t)i * SPLAT_REC];
        const float nx = (rec.x - 0.5f * (float)(W - 1)) / (0.5f * (float)W), ny = (rec.y - 0.5f * (float)(H - 1)) / (0.5f * (float)H);
        c_x = acc[0] * nx + 2.f * a0 * dL_da + b * dL_db;
        c_y = acc[1] * ny + 2.f * c0 * dL_dc + b * dL_db;
    }
    if (per_splat != nullptr && i < P) {
        per_splat[2 * (size_t)i] = c_x;
        per_splat[2 * (size_t)i + 1] = c_y;
    }
    red[0][threadIdx.x] = c_x;
    red[1][threadIdx.x] = c_y;
    focal_tree_sum(red);
    if (threadIdx.x < 2) block_rows[2 * (size_t)blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

// one workgroup: thread t adds the rows t, t + 256, .. in index order, then the same tree
__global__ void __launch_bounds__(256) focal_finish_kernel(int nrows, const float *__restrict__ block_rows, float *__restrict__ sums) {
    __shared__ float red[2][256];
    float s0 = 0.f, s1 = 0.f;
    for (int r = threadIdx.x; r < nrows; r += 256) {
        s0 += block_rows[2 * (size_t)r];
        s1 += block_rows[2 * (size_t)r + 1];
    }
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    focal_tree_sum(red);
    if (threadIdx.x < 2) sums[threadIdx.x] = red[threadIdx.x][0];
}

size_t focal_workspace_bytes(int P) { return (size_t)std::max(div_up(P > 0 ? P : 0, 256), 1) * 2 * sizeof(float); }

int launch_focal_grad(const das3r_raster_args *a, const das3r_raster_in *in, const char *geom, const Layout &L, const float *partial, bool quad_rows,
                      bool aa, float *sums, float *per_splat, float *workspace, hipStream_t s) {
    const int P = a->P;
    const int blocks = div_up(P, 256);
    const size_t cap_rows = L.capacity > 0 ? (size_t)L.capacity : 1;
    const uint8_t *exists = quad_rows ? reinterpret_cast<const uint8_t *>(partial) + align_up(cap_rows * 4 * 12 * sizeof(float)) : nullptr;
    const PreXform pre = pre_xform(in);
#define ARGS                                                                                                                              \
    P, in->means3D, in->scales, a->scale_modifier, in->rotations, in->cov3D_precomp, in->opacities, pre, a->viewmatrix, a->image_width,   \
        a->image_height, a->tanfovx, a->tanfovy, (const uint32_t *)(geom + L.pub.tiles_touched), (const uint32_t *)(geom + L.g_off_by_gid), \
        (const float4 *)(geom + L.pub.xy), partial, exists, per_splat, workspace
    if (in->cov3D_precomp) {
        if (aa) DAS3R_LAUNCH((focal_grad_kernel<true, true>), dim3(blocks), dim3(256), 0, s, ARGS);
        else DAS3R_LAUNCH((focal_grad_kernel<true, false>), dim3(blocks), dim3(256), 0, s, ARGS);
    } else {
        if (aa) DAS3R_LAUNCH((focal_grad_kernel<false, true>), dim3(blocks), dim3(256), 0, s, ARGS);
        else DAS3R_LAUNCH((focal_grad_kernel<false, false>), dim3(blocks), dim3(256), 0, s, ARGS);
    }
#undef ARGS
    KERNEL_CHECK(s, a->debug, "focal_grad");
    DAS3R_LAUNCH(focal_finish_kernel, dim3(1), dim3(256), 0, s, blocks, workspace, sums);
    KERNEL_CHECK(s, a->debug, "focal_finish");
    return DAS3R_OK;
}

}  // namespace das3r
