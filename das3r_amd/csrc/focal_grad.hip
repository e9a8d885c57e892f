// focal_grad.hip — dL/d(log-focal offsets) of a backward pass (das3r_raster_backward_focal, api.hip): one per-Gaussian kernel between the
// compositing backward and the per-Gaussian backward, where depth_fold_kernel sits.
//
// s = (s_x, s_y): the forward at s is the forward with tanfovx e^(-s_x), tanfovy e^(-s_y) and the clip-x / clip-y columns of projmatrix
// scaled by e^(s_x) / e^(s_y).  With every discrete decision held fixed (cull, radius, rectangle, lists, the 1/255 and T < 1e-4 cut-offs, the
// EWA clamp flags; the clamped ray a constant, as upstream treats it for the mean) a splat's pixel mean moves as
// (u - (W - 1) / 2) e^(s_x), its undilated covariance as a0 e^(2 s_x), b e^(s_x + s_y), c0 e^(2 s_y); the SH view direction and 1/z do not move.
// So, per rendered splat, from the row sums the compositing backward left (partial[], the rows off_by_gid[i] .. + tiles_touched[i]):
//   c_x = dL/du (u - (W - 1) / 2) + 2 a0 dL/da + b dL/db        c_y = dL/dv (v - (H - 1) / 2) + 2 c0 dL/dc + b dL/db
// with dL/d(a, b, c) preprocess_backward_kernel's — the same function, splat_math.h conic_grad_to_cov2d, the antialiasing factor's term
// included — and dL/ds = sum_i c(i).
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
        sum_instance_rows<3, 6, true>(partial, row_exists, off_by_gid[i], n, acc);
        // the forward's inputs again (pretransform_math.h: the same bits), its T and its undilated covariance
        float3 mean, sc;
        float4 q;
        float c3[6];
        RawGeometry raw;
        float op_in = 0.f;   // (AA only)
        load_forward_inputs<HAS_COV, AA>(pre, false, means3D, scales, rotations, opacities, cov3D_precomp, i, mean, sc, q, c3, op_in, raw);
        if constexpr (!HAS_COV) cov3d_from_scale_rot(sc, scale_modifier, q, c3);
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
        // ---- conic sums -> dL/d(a, b, c): preprocess_backward_kernel's, by the functions it calls (splat_math.h)
        const float ca = a0 + 0.3f, cc = c0 + 0.3f;
        const float gA = acc[2], gB = acc[3], gC = acc[4];
        const float denom = ca * cc - b * b;
        float aa_r = 0.f, aa_drho = 0.f;
        if constexpr (AA) {
            aa_r = aa_rho(a0, b, c0, denom);
            const float f = aa_factor(aa_r);
            aa_drho = aa_opacity_grad_to_rho(aa_r, f, acc[5], op_in);
        }
        float dL_da = 0.f, dL_db = 0.f, dL_dc = 0.f;
        const float denom2inv = 1.0f / ((denom * denom) + 0.0000001f);
        if (denom2inv != 0.f) conic_grad_to_cov2d<AA>(gA, gB, gC, ca, b, cc, a0, c0, denom, denom2inv, aa_r, aa_drho, dL_da, dL_db, dL_dc);
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

int launch_focal_grad(const das3r_raster_args *a, const das3r_raster_in *in, const Buffers &v, const float *partial, bool quad_rows,
                      bool aa, float *sums, float *per_splat, float *workspace, hipStream_t s) {
    const int P = a->P;
    const int blocks = div_up(P, 256);
    const uint8_t *exists = quad_rows_exist(partial, v.L, quad_rows);
    const PreXform pre = pre_xform(in);
#define ARGS                                                                                                                              \
    P, in->means3D, in->scales, a->scale_modifier, in->rotations, in->cov3D_precomp, in->opacities, pre, a->viewmatrix, a->image_width,   \
        a->image_height, a->tanfovx, a->tanfovy, v.tiles_touched(), v.g_off_by_gid(), v.xy(), partial, exists, per_splat, workspace
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
