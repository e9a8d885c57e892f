// normals.hip — the normal-consistency regulariser's two halves that are no walk over tile lists (include/das3r_raster.h
// das3r_gaussian_normals_forward / _backward, das3r_normal_consistency_forward / _backward: the definitions are fixed there, word for word).
//
// 1. Per-Gaussian normals: one thread per Gaussian, streaming (40 B in, 13 B out forward; 29 B in, 16 B out backward), no LDS, no atomics.
//    The unit is built with the EXACT rule of the Makefile (no FMA contraction): k = argmin scale and flip = (a . d > 0) are plain IEEE fp32.
// 2. The depth image's normal and the loss against the blended normal: a stencil.  A workgroup takes a 32 x 8 tile of pixels and stages the
//    depths of the tile and its halo in LDS — every halo index clamped into the image BEFORE the load, so nothing outside the image is read; a
//    clamped copy is never used, because the only pixels whose stencil would reach it are border pixels, which are invalid by definition.
//    The backward is in GATHER form: output pixel q adds what its four neighbours' stencils send to z_q, recomputing each neighbour's cross
//    product from the staged radius-2 diamond.  No floating-point atomics, nothing pre-zeroed, every output word written, bit-identical runs.
#include <math.h>

#include "common.h"

namespace das3r {

// ------------------------------------------------------------------------------------------------------------------ 1. per-Gaussian normals

// column k of R(q), q = (r, x, y, z) a UNIT quaternion: the matrix include/das3r_raster.h spells out (splat_math.h builds the same one)
__device__ __forceinline__ float3 rot_column(const float r, const float x, const float y, const float z, const int k) {
    if (k == 0) return make_float3(1.f - 2.f * (y * y + z * z), 2.f * (x * y + r * z), 2.f * (x * z - r * y));
    if (k == 1) return make_float3(2.f * (x * y - r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z + r * x));
    return make_float3(2.f * (x * z + r * y), 2.f * (y * z - r * x), 1.f - 2.f * (x * x + y * y));
}

// 1 / |q|, or 0 for a quaternion whose norm is 0 or not finite (its normal and its gradient are then exact zeros)
__device__ __forceinline__ float quat_inv_norm(const float r, const float x, const float y, const float z) {
    const float n2 = r * r + x * x + y * y + z * z;
    return (n2 > 0.f && n2 < INFINITY) ? 1.0f / sqrtf(n2) : 0.f;
}

__global__ void __launch_bounds__(256) gaussian_normals_forward_kernel(int P, const float *__restrict__ rotations, const float *__restrict__ scales,
                                                                       const float *__restrict__ means3D, const float *__restrict__ viewmatrix,
                                                                       const float *__restrict__ campos, float *__restrict__ normals,
                                                                       uint8_t *__restrict__ choice) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
    const float s0 = scales[i3], s1 = scales[i3 + 1], s2 = scales[i3 + 2];
    int k = 0;   // argmin, ties to the lowest index
    float smin = s0;
    if (s1 < smin) { k = 1; smin = s1; }
    if (s2 < smin) { k = 2; }
    float r = rotations[i4], x = rotations[i4 + 1], y = rotations[i4 + 2], z = rotations[i4 + 3];
    const float inv = quat_inv_norm(r, x, y, z);
    r *= inv, x *= inv, y *= inv, z *= inv;
    float3 a = inv != 0.f ? rot_column(r, x, y, z, k) : make_float3(0.f, 0.f, 0.f);
    const float dx = means3D[i3] - campos[0], dy = means3D[i3 + 1] - campos[1], dz = means3D[i3 + 2] - campos[2];
    const float dot = a.x * dx + a.y * dy + a.z * dz;
    const bool flip = dot > 0.f;   // (exactly 0, or NaN: a is kept)
    if (flip) a = make_float3(-a.x, -a.y, -a.z);
    // into view space by the rotation part of viewmatrix, row-vector convention (splat_math.h xform43 without the translation)
    const float *m = viewmatrix;
    normals[i3] = m[0] * a.x + m[4] * a.y + m[8] * a.z;
    normals[i3 + 1] = m[1] * a.x + m[5] * a.y + m[9] * a.z;
    normals[i3 + 2] = m[2] * a.x + m[6] * a.y + m[10] * a.z;
    choice[i] = (uint8_t)(k | ((flip ? 1 : 0) << 2));
}

template <bool ACCUMULATE>
__global__ void __launch_bounds__(256) gaussian_normals_backward_kernel(int P, const float *__restrict__ rotations, const uint8_t *__restrict__ choice,
                                                                        const float *__restrict__ viewmatrix, const float *__restrict__ dL_dnormals,
                                                                        float *__restrict__ dL_drotations) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const size_t i3 = 3 * (size_t)i, i4 = 4 * (size_t)i;
    const uint8_t ch = choice[i];
    const int k = ch & 3;
    const bool flip = (ch & 4) != 0;
    float r = rotations[i4], x = rotations[i4 + 1], y = rotations[i4 + 2], z = rotations[i4 + 3];
    const float inv = quat_inv_norm(r, x, y, z);
    r *= inv, x *= inv, y *= inv, z *= inv;
    // view -> world: the transpose of the forward's product; then the flip
    const float *m = viewmatrix;
    const float gx = dL_dnormals[i3], gy = dL_dnormals[i3 + 1], gz = dL_dnormals[i3 + 2];
    float ax = m[0] * gx + m[1] * gy + m[2] * gz, ay = m[4] * gx + m[5] * gy + m[6] * gz, az = m[8] * gx + m[9] * gy + m[10] * gz;
    if (flip) ax = -ax, ay = -ay, az = -az;
    // dL/d(unit quaternion): the column's derivative
    float gr, gqx, gqy, gqz;
    if (k == 0) {   // a = (1 - 2 (y^2 + z^2), 2 (x y + r z), 2 (x z - r y))
        gr = 2.f * (z * ay - y * az);
        gqx = 2.f * (y * ay + z * az);
        gqy = -4.f * y * ax + 2.f * (x * ay - r * az);
        gqz = -4.f * z * ax + 2.f * (r * ay + x * az);
    } else if (k == 1) {   // a = (2 (x y - r z), 1 - 2 (x^2 + z^2), 2 (y z + r x))
        gr = 2.f * (x * az - z * ax);
        gqx = 2.f * (y * ax + r * az) - 4.f * x * ay;
        gqy = 2.f * (x * ax + z * az);
        gqz = 2.f * (y * az - r * ax) - 4.f * z * ay;
    } else {   // a = (2 (x z + r y), 2 (y z - r x), 1 - 2 (x^2 + y^2))
        gr = 2.f * (y * ax - x * ay);
        gqx = 2.f * (z * ax - r * ay) - 4.f * x * az;
        gqy = 2.f * (r * ax + z * ay) - 4.f * y * az;
        gqz = 2.f * (x * ax + y * ay);
    }
    // through q / |q|: (g - q^ (q^ . g)) / |q|
    const float qg = r * gr + x * gqx + y * gqy + z * gqz;
    float o0 = (gr - r * qg) * inv, o1 = (gqx - x * qg) * inv, o2 = (gqy - y * qg) * inv, o3 = (gqz - z * qg) * inv;
    if (inv == 0.f) o0 = o1 = o2 = o3 = 0.f;   // (no norm, no axis: selected, an infinite component times 0 is NaN)
    if (ACCUMULATE) {
        dL_drotations[i4] += o0, dL_drotations[i4 + 1] += o1, dL_drotations[i4 + 2] += o2, dL_drotations[i4 + 3] += o3;
    } else {
        dL_drotations[i4] = o0, dL_drotations[i4 + 1] = o1, dL_drotations[i4 + 2] = o2, dL_drotations[i4 + 3] = o3;
    }
}

// ------------------------------------------------------------------------------------------------- 2. depth normals and the loss image

constexpr int NC_TX = 32, NC_TY = 8, NC_THREADS = NC_TX * NC_TY;

// the depths of the tile at (x0, y0) and its HALO-pixel frame -> tile[(NC_TY + 2 HALO)][(NC_TX + 2 HALO)]; every index clamped into the image
template <int HALO>
__device__ __forceinline__ void stage_depth_tile(const float *__restrict__ depth, const int W, const int H, const int x0, const int y0,
                                                 float (&tile)[NC_TY + 2 * HALO][NC_TX + 2 * HALO]) {
    constexpr int TW = NC_TX + 2 * HALO, TH = NC_TY + 2 * HALO;
    for (int c = threadIdx.x; c < TW * TH; c += NC_THREADS) {
        const int j = c / TW, i = c - j * TW;
        const int x = min(max(x0 - HALO + i, 0), W - 1), y = min(max(y0 - HALO + j, 0), H - 1);
        tile[j][i] = depth[(size_t)y * W + x];
    }
    __syncthreads();
}

struct Camera2 {
    int W, H;
    float tanfovx, tanfovy;
};

__device__ __forceinline__ bool depth_ok(const float z) { return z > 0.f && z < INFINITY; }   // finite and > 0 (NaN fails both)

// The stencil of pixel (x, y): tangents dx, dy (the non-cancelling central differences), c = dy x dx, inv = 1 / |c|.  -> the pixel is valid.
// (x, y) may lie outside the image: that is an invalid pixel.
struct Stencil {
    float3 dx, dy, c;
    float inv, rx, ry, tx, ty;
};
__device__ __forceinline__ bool pixel_stencil(const Camera2 cam, const int x, const int y, const float zc, const float zl, const float zr,
                                              const float zu, const float zd, Stencil &s) {
    if (x < 1 || y < 1 || x > cam.W - 2 || y > cam.H - 2) return false;
    if (!(depth_ok(zc) && depth_ok(zl) && depth_ok(zr) && depth_ok(zu) && depth_ok(zd))) return false;
    s.rx = ((float)(2 * x + 1) / (float)cam.W - 1.f) * cam.tanfovx;
    s.ry = ((float)(2 * y + 1) / (float)cam.H - 1.f) * cam.tanfovy;
    s.tx = 2.f * cam.tanfovx / (float)cam.W;   // the ray's step from one pixel to the next
    s.ty = 2.f * cam.tanfovy / (float)cam.H;
    const float ex = zr - zl, ey = zd - zu;
    s.dx = make_float3(ex * s.rx + (zr + zl) * s.tx, ex * s.ry, ex);
    s.dy = make_float3(ey * s.rx, ey * s.ry + (zd + zu) * s.ty, ey);
    s.c = make_float3(s.dy.y * s.dx.z - s.dy.z * s.dx.y, s.dy.z * s.dx.x - s.dy.x * s.dx.z, s.dy.x * s.dx.y - s.dy.y * s.dx.x);
    const float n2 = s.c.x * s.c.x + s.c.y * s.c.y + s.c.z * s.c.z;
    if (!(n2 > 0.f && n2 < INFINITY)) return false;
    s.inv = 1.0f / sqrtf(n2);
    return true;
}

__global__ void __launch_bounds__(NC_THREADS) normal_consistency_forward_kernel(const Camera2 cam, const int tiles_x, const float *__restrict__ depth,
                                                                                const float *__restrict__ normal, const float *__restrict__ alpha,
                                                                                const float *__restrict__ mask, float *__restrict__ loss,
                                                                                float *__restrict__ depth_normal) {
    __shared__ float tile[NC_TY + 2][NC_TX + 2];
    const int W = cam.W, H = cam.H;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * NC_TX, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * NC_TY;
    stage_depth_tile<1>(depth, W, H, x0, y0, tile);
    const int lx = threadIdx.x % NC_TX, ly = threadIdx.x / NC_TX;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const size_t npix = (size_t)W * H, p = (size_t)y * W + x;
    Stencil s;
    const bool valid = pixel_stencil(cam, x, y, tile[ly + 1][lx + 1], tile[ly + 1][lx], tile[ly + 1][lx + 2], tile[ly][lx + 1], tile[ly + 2][lx + 1], s);
    float out = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (valid) {
        nx = s.c.x * s.inv, ny = s.c.y * s.inv, nz = s.c.z * s.inv;
        const float m = mask != nullptr ? mask[p] : 1.f;
        out = m * (alpha[p] - (normal[p] * nx + normal[npix + p] * ny + normal[2 * npix + p] * nz));
    }
    loss[p] = out;
    if (depth_normal != nullptr) {
        depth_normal[p] = nx;
        depth_normal[npix + p] = ny;
        depth_normal[2 * npix + p] = nz;
    }
}

// What the stencil of pixel (x, y) — depths from the staged tile, cell (i, j) = the pixel's own — sends to its four neighbours' depths for
// the upstream gradient g of its loss: gz[0..3] = dL/d(z_left, z_right, z_up, z_down).  An invalid pixel (outside the image included) sends 0.
template <int TW, int TH>
__device__ __forceinline__ void stencil_depth_grads(const Camera2 cam, const int x, const int y, const float (&tile)[TH][TW], const int i, const int j,
                                                    const float *__restrict__ normal, const float *__restrict__ mask,
                                                    const float *__restrict__ dL_dloss, float (&gz)[4]) {
    gz[0] = gz[1] = gz[2] = gz[3] = 0.f;
    Stencil s;
    if (!pixel_stencil(cam, x, y, tile[j][i], tile[j][i - 1], tile[j][i + 1], tile[j - 1][i], tile[j + 1][i], s)) return;
    const size_t npix = (size_t)cam.W * cam.H, p = (size_t)y * cam.W + x;   // (valid: inside the image)
    const float gm = dL_dloss[p] * (mask != nullptr ? mask[p] : 1.f);
    // loss = m (alpha - n . N), N = c / |c|:  dL/dN = -g m n,  dL/dc = (dL/dN - N (N . dL/dN)) / |c|
    const float Nx = s.c.x * s.inv, Ny = s.c.y * s.inv, Nz = s.c.z * s.inv;
    const float hx = -gm * normal[p], hy = -gm * normal[npix + p], hz = -gm * normal[2 * npix + p];
    const float Nh = Nx * hx + Ny * hy + Nz * hz;
    const float cx = (hx - Nx * Nh) * s.inv, cy = (hy - Ny * Nh) * s.inv, cz = (hz - Nz * Nh) * s.inv;
    // c = dy x dx:  dL/d(dy) = dx x dL/dc,  dL/d(dx) = dL/dc x dy
    const float ux = s.dx.y * cz - s.dx.z * cy, uy = s.dx.z * cx - s.dx.x * cz, uz = s.dx.x * cy - s.dx.y * cx;   // dL/d(dy)
    const float vx = cy * s.dy.z - cz * s.dy.y, vy = cz * s.dy.x - cx * s.dy.z, vz = cx * s.dy.y - cy * s.dy.x;   // dL/d(dx)
    // d(dx)/dz_right = (rx + tx, ry, 1), d(dx)/dz_left = (-rx + tx, -ry, -1); d(dy)/dz_down = (rx, ry + ty, 1), d(dy)/dz_up = (-rx, -ry + ty, -1)
    const float along_x = vx * s.rx + vy * s.ry + vz, along_y = ux * s.rx + uy * s.ry + uz;
    gz[0] = vx * s.tx - along_x;
    gz[1] = vx * s.tx + along_x;
    gz[2] = uy * s.ty - along_y;
    gz[3] = uy * s.ty + along_y;
}

__global__ void __launch_bounds__(NC_THREADS) normal_consistency_backward_kernel(const Camera2 cam, const int tiles_x, const float *__restrict__ depth,
                                                                                 const float *__restrict__ normal, const float *__restrict__ mask,
                                                                                 const float *__restrict__ dL_dloss, float *__restrict__ dL_ddepth,
                                                                                 float *__restrict__ dL_dnormal, float *__restrict__ dL_dalpha) {
    constexpr int TW = NC_TX + 4, TH = NC_TY + 4;
    __shared__ float tile[TH][TW];
    const int W = cam.W, H = cam.H;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * NC_TX, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * NC_TY;
    stage_depth_tile<2>(depth, W, H, x0, y0, tile);
    const int lx = threadIdx.x % NC_TX, ly = threadIdx.x / NC_TX;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const size_t npix = (size_t)W * H, p = (size_t)y * W + x;
    const int i = lx + 2, j = ly + 2;
    // the pixel's own stencil: dL/dalpha and dL/dnormal
    Stencil s;
    float ga = 0.f, gnx = 0.f, gny = 0.f, gnz = 0.f;
    if (pixel_stencil(cam, x, y, tile[j][i], tile[j][i - 1], tile[j][i + 1], tile[j - 1][i], tile[j + 1][i], s)) {
        ga = dL_dloss[p] * (mask != nullptr ? mask[p] : 1.f);
        gnx = -ga * (s.c.x * s.inv), gny = -ga * (s.c.y * s.inv), gnz = -ga * (s.c.z * s.inv);
    }
    dL_dalpha[p] = ga;
    dL_dnormal[p] = gnx;
    dL_dnormal[npix + p] = gny;
    dL_dnormal[2 * npix + p] = gnz;
    // the four neighbours whose stencils read z here, in a fixed order: left neighbour (this is its right), right, upper, lower
    float gz[4];
    float acc = 0.f;
    stencil_depth_grads<TW, TH>(cam, x - 1, y, tile, i - 1, j, normal, mask, dL_dloss, gz);
    acc += gz[1];
    stencil_depth_grads<TW, TH>(cam, x + 1, y, tile, i + 1, j, normal, mask, dL_dloss, gz);
    acc += gz[0];
    stencil_depth_grads<TW, TH>(cam, x, y - 1, tile, i, j - 1, normal, mask, dL_dloss, gz);
    acc += gz[3];
    stencil_depth_grads<TW, TH>(cam, x, y + 1, tile, i, j + 1, normal, mask, dL_dloss, gz);
    acc += gz[2];
    dL_ddepth[p] = acc;
}

}  // namespace das3r

using namespace das3r;

extern "C" int das3r_gaussian_normals_forward(const das3r_raster_args *args, const float *rotations, const float *scales, const float *means3D,
                                              float *normals, uint8_t *choice, das3r_stream_t stream) {
    const char *who = "das3r_gaussian_normals_forward";
    if (!args) { set_error("%s: null args", who); return DAS3R_ERR_INVALID_ARG; }
    if (args->P < 0) { set_error("%s: P = %d", who, args->P); return DAS3R_ERR_INVALID_ARG; }
    if (args->P == 0) return DAS3R_OK;
    if (!args->viewmatrix || !args->campos) { set_error("%s: null args->viewmatrix / args->campos", who); return DAS3R_ERR_INVALID_ARG; }
    if (!rotations || !scales || !means3D) { set_error("%s: null rotations / scales / means3D (a cov3D_precomp caller has no axes)", who); return DAS3R_ERR_INVALID_ARG; }
    if (!normals || !choice) { set_error("%s: null normals / choice", who); return DAS3R_ERR_INVALID_ARG; }
    hipStream_t s = (hipStream_t)stream;
    DAS3R_LAUNCH(gaussian_normals_forward_kernel, dim3(div_up(args->P, 256)), dim3(256), 0, s, args->P, rotations, scales, means3D, args->viewmatrix,
                 args->campos, normals, choice);
    KERNEL_CHECK(s, args->debug, "gaussian_normals_forward");
    return DAS3R_OK;
}

extern "C" int das3r_gaussian_normals_backward(const das3r_raster_args *args, const float *rotations, const uint8_t *choice, const float *dL_dnormals,
                                               float *dL_drotations, int32_t accumulate, das3r_stream_t stream) {
    const char *who = "das3r_gaussian_normals_backward";
    if (!args) { set_error("%s: null args", who); return DAS3R_ERR_INVALID_ARG; }
    if (args->P < 0) { set_error("%s: P = %d", who, args->P); return DAS3R_ERR_INVALID_ARG; }
    if (args->P == 0) return DAS3R_OK;
    if (!args->viewmatrix) { set_error("%s: null args->viewmatrix", who); return DAS3R_ERR_INVALID_ARG; }
    if (!rotations || !choice) { set_error("%s: null rotations / choice (the forward call's)", who); return DAS3R_ERR_INVALID_ARG; }
    if (!dL_dnormals || !dL_drotations) { set_error("%s: null dL_dnormals / dL_drotations", who); return DAS3R_ERR_INVALID_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(div_up(args->P, 256));
    if (accumulate)
        DAS3R_LAUNCH(gaussian_normals_backward_kernel<true>, grid, dim3(256), 0, s, args->P, rotations, choice, args->viewmatrix, dL_dnormals, dL_drotations);
    else
        DAS3R_LAUNCH(gaussian_normals_backward_kernel<false>, grid, dim3(256), 0, s, args->P, rotations, choice, args->viewmatrix, dL_dnormals, dL_drotations);
    KERNEL_CHECK(s, args->debug, "gaussian_normals_backward");
    return DAS3R_OK;
}

// the checks both image entries share -> DAS3R_OK, or the refusal (message set)
static int check_image_call(const char *who, int32_t H, int32_t W, float tanfovx, float tanfovy) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > ((int64_t)1 << 30)) { set_error("%s: bad extents H=%d W=%d (H, W > 0, H * W <= 2^30)", who, H, W); return DAS3R_ERR_INVALID_ARG; }
    if (!isfinite(tanfovx) || !isfinite(tanfovy)) { set_error("%s: tanfovx / tanfovy must be finite (got %g, %g)", who, (double)tanfovx, (double)tanfovy); return DAS3R_ERR_INVALID_ARG; }
    return DAS3R_OK;
}

extern "C" int das3r_normal_consistency_forward(int32_t H, int32_t W, float tanfovx, float tanfovy, const float *depth, const float *normal,
                                                const float *alpha, const float *mask, float *loss, float *depth_normal, das3r_stream_t stream) {
    const char *who = "das3r_normal_consistency_forward";
    if (const int rc = check_image_call(who, H, W, tanfovx, tanfovy)) return rc;
    if (!depth || !normal || !alpha || !loss) { set_error("%s: null depth / normal / alpha / loss (mask and depth_normal may be NULL)", who); return DAS3R_ERR_INVALID_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const Camera2 cam = {W, H, tanfovx, tanfovy};
    const int tiles_x = div_up(W, NC_TX), tiles_y = div_up(H, NC_TY);
    DAS3R_LAUNCH(normal_consistency_forward_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(NC_THREADS), 0, s, cam, tiles_x, depth, normal, alpha,
                 mask, loss, depth_normal);
    KERNEL_CHECK(s, false, "normal_consistency_forward");
    return DAS3R_OK;
}

extern "C" int das3r_normal_consistency_backward(int32_t H, int32_t W, float tanfovx, float tanfovy, const float *depth, const float *normal,
                                                 const float *mask, const float *dL_dloss, float *dL_ddepth, float *dL_dnormal, float *dL_dalpha,
                                                 das3r_stream_t stream) {
    const char *who = "das3r_normal_consistency_backward";
    if (const int rc = check_image_call(who, H, W, tanfovx, tanfovy)) return rc;
    if (!depth || !normal || !dL_dloss) { set_error("%s: null depth / normal / dL_dloss (mask may be NULL)", who); return DAS3R_ERR_INVALID_ARG; }
    if (!dL_ddepth || !dL_dnormal || !dL_dalpha) { set_error("%s: null dL_ddepth / dL_dnormal / dL_dalpha", who); return DAS3R_ERR_INVALID_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const Camera2 cam = {W, H, tanfovx, tanfovy};
    const int tiles_x = div_up(W, NC_TX), tiles_y = div_up(H, NC_TY);
    DAS3R_LAUNCH(normal_consistency_backward_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(NC_THREADS), 0, s, cam, tiles_x, depth, normal, mask,
                 dL_dloss, dL_ddepth, dL_dnormal, dL_dalpha);
    KERNEL_CHECK(s, false, "normal_consistency_backward");
    return DAS3R_OK;
}
