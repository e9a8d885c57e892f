// depth_loss.hip — the inverse-depth L1 term of a depth-supervised train step (INTEGRATION.md "Depth supervision"), value and gradient in
// one sweep over the pixels:
//     L_depth_pure = mean over all H*W pixels of |(D - D*) m s|          (upstream 3DGS: torch.abs((invDepth - mono_invdepth) * depth_mask).mean())
//     d_invdepth   = grad_loss * w * m s * sgn((D - D*) m s) / (H W)     (sgn(0) = 0)
// D: the rasterizer's inverse-depth image (ABI 16 out_invdepth), D*: the target, m: the validity mask, s: the frame's static mask taken as
// a constant (null = 1), w: the schedule's weight.  A pixel with m s == 0 gives exactly 0 to value and gradient whatever D* holds there.
//
// Two launches, both tiny (the image is ~106 k pixels: this is launch latency, not bandwidth).  The first: 256 threads x four consecutive
// pixels each (one float4 per array where the extents and pointers allow), every workgroup leaves ONE partial sum; the second: one
// workgroup adds those rows in index order and writes the three values into the step's out8.  No floating-point atomics and no arrival
// counter: the sum has one order, the same from run to run, and nothing has to be zero or re-armed between calls.
#include "common.h"

namespace das3r {

constexpr int DL_THREADS = 256, DL_PER_THREAD = 4, DL_PER_BLOCK = DL_THREADS * DL_PER_THREAD;

// sum of `v` over the workgroup's 256 threads, valid in thread 0 (red: float[4] LDS)
__device__ __forceinline__ float block_sum_256(float v, float *red) {
    const int lane = __lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

template <bool VEC>
__global__ void __launch_bounds__(DL_THREADS) depth_l1_kernel(int npix, const float *__restrict__ invdepth, const float *__restrict__ target,
                                                              const float *__restrict__ mask, const float *__restrict__ stat, float weight,
                                                              const float *__restrict__ grad_loss, float *__restrict__ d_invdepth,
                                                              float *__restrict__ partials /*[blocks][8]*/) {
    __shared__ float red[4];
    const int p0 = (blockIdx.x * DL_THREADS + threadIdx.x) * DL_PER_THREAD;
    const float scale = weight * (grad_loss != nullptr ? grad_loss[0] : 1.f) / (float)npix;
    float D[4], T[4], M[4], S[4] = {1.f, 1.f, 1.f, 1.f};
    if (VEC) {   // (npix % 4 == 0 and 16-byte aligned pointers: the four pixels are all inside or all outside)
        const bool in = p0 < npix;
        const int q = in ? p0 >> 2 : 0;
        const float4 d4 = reinterpret_cast<const float4 *>(invdepth)[q], t4 = reinterpret_cast<const float4 *>(target)[q];
        const float4 m4 = reinterpret_cast<const float4 *>(mask)[q];
        D[0] = d4.x, D[1] = d4.y, D[2] = d4.z, D[3] = d4.w;
        T[0] = t4.x, T[1] = t4.y, T[2] = t4.z, T[3] = t4.w;
        M[0] = in ? m4.x : 0.f, M[1] = in ? m4.y : 0.f, M[2] = in ? m4.z : 0.f, M[3] = in ? m4.w : 0.f;
        if (stat != nullptr) {
            const float4 s4 = reinterpret_cast<const float4 *>(stat)[q];
            S[0] = s4.x, S[1] = s4.y, S[2] = s4.z, S[3] = s4.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool in = p0 + k < npix;
            const int p = in ? p0 + k : 0;
            D[k] = invdepth[p], T[k] = target[p];
            M[k] = in ? mask[p] : 0.f;
            if (stat != nullptr) S[k] = stat[p];
        }
    }
    float acc = 0.f, g[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float ms = M[k] * S[k];
        const float e = (D[k] - T[k]) * ms;
        const bool off = ms == 0.f;   // (not `e == 0`: a NaN target behind a zero mask must not reach value or gradient)
        acc += off ? 0.f : fabsf(e);
        g[k] = off ? 0.f : scale * ms * (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f));
    }
    if (VEC) {
        if (p0 < npix) reinterpret_cast<float4 *>(d_invdepth)[p0 >> 2] = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (p0 + k < npix) d_invdepth[p0 + k] = g[k];
    }
    const float total = block_sum_256(acc, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.x * 8] = total;
}

// the rows of the kernel above, added in index order -> out8[5] = L_depth_pure, out8[6] = w L_depth_pure, out8[0] += w L_depth_pure
__global__ void __launch_bounds__(DL_THREADS) depth_l1_finish_kernel(int nblocks, const float *__restrict__ partials, float npix, float weight,
                                                                     float *__restrict__ out8) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int b = threadIdx.x; b < nblocks; b += DL_THREADS) acc += partials[(size_t)b * 8];
    const float total = block_sum_256(acc, red);
    if (threadIdx.x == 0) {
        const float pure = total / npix, weighted = weight * pure;
        out8[5] = pure;
        out8[6] = weighted;
        out8[0] += weighted;
    }
}

}  // namespace das3r

using namespace das3r;

extern "C" int64_t das3r_depth_l1_blocks(int32_t H, int32_t W) {
    if (H <= 0 || W <= 0) return 0;
    return ((int64_t)H * W + DL_PER_BLOCK - 1) / DL_PER_BLOCK;
}

extern "C" int das3r_depth_l1(int32_t H, int32_t W, const float *invdepth, const float *target, const float *mask, const float *static_mask,
                              float weight, const float *grad_loss, float *d_invdepth, float *partials, float *out8, das3r_stream_t stream) {
    if (H <= 0 || W <= 0 || (int64_t)H * W > (int64_t)(1 << 30) || !invdepth || !target || !mask || !d_invdepth || !partials || !out8) {
        set_error("das3r_depth_l1: invalid argument (H, W > 0, H * W <= 2^30; invdepth, target, mask, d_invdepth, partials, out8 must not be NULL)");
        return DAS3R_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int npix = H * W, nb = (int)das3r_depth_l1_blocks(H, W);
    const uintptr_t bits = (uintptr_t)invdepth | (uintptr_t)target | (uintptr_t)mask | (uintptr_t)static_mask | (uintptr_t)d_invdepth;
    if (npix % 4 == 0 && bits % 16 == 0)
        DAS3R_LAUNCH(depth_l1_kernel<true>, dim3(nb), dim3(DL_THREADS), 0, s, npix, invdepth, target, mask, static_mask, weight, grad_loss, d_invdepth, partials);
    else
        DAS3R_LAUNCH(depth_l1_kernel<false>, dim3(nb), dim3(DL_THREADS), 0, s, npix, invdepth, target, mask, static_mask, weight, grad_loss, d_invdepth, partials);
    KERNEL_CHECK(s, false, "depth_l1");
    DAS3R_LAUNCH(depth_l1_finish_kernel, dim3(1), dim3(DL_THREADS), 0, s, nb, partials, (float)npix, weight, out8);
    KERNEL_CHECK(s, false, "depth_l1_finish");
    return DAS3R_OK;
}
