// pretransform_math.h — the pose pre-transform of a Gaussian (/root/reference/gaussian_renderer/__init__.py:83-97,107)
// as ONE piece of arithmetic, shared by pretransform_forward_kernel (pretransform.hip: writes the camera-frame tensors) and by the
// per-Gaussian kernels of the rasterizer when the caller hands them the raw parameters instead (das3r_raster_in.pre, round 6: the
// camera-frame means / rotations / scales / opacities then never reach HBM — preprocess.hip, preprocess_bwd.hip).  Every operation is spelled
// out (explicit fused multiply-adds, rounded products): the translation units that include this are compiled with different contraction
// flags, and the three kernels must produce the same bits.
#pragma once
#include <stdint.h>

namespace das3r {

struct PreXform {   // device-side view of include/das3r_raster.h das3r_pretransform (xyz == nullptr: not in use)
    const float *xyz, *rot, *scaling, *opacity_raw, *conf_flat;
    const int64_t *mask_index;
    const float *Rm, *tv, *Lq;
};

#ifdef __HIPCC__
struct PoseRegs { float R[9], t[3], L[16]; };
__device__ __forceinline__ void load_pose(const float *__restrict__ Rm, const float *__restrict__ tv, const float *__restrict__ Lq, PoseRegs &p) {
#pragma unroll
    for (int i = 0; i < 9; i++) p.R[i] = Rm[i];
#pragma unroll
    for (int i = 0; i < 3; i++) p.t[i] = tv[i];
#pragma unroll
    for (int i = 0; i < 16; i++) p.L[i] = Lq[i];
}
__device__ __forceinline__ float pre_dot3(const float a, const float b, const float c, const float x, const float y, const float z, const float t) {
    return __fadd_rn(__fmaf_rn(c, z, __fmaf_rn(b, y, __fmul_rn(a, x))), t);
}
__device__ __forceinline__ float pre_dot4(const float a, const float b, const float c, const float d, const float4 q) {
    return __fmaf_rn(d, q.w, __fmaf_rn(c, q.z, __fmaf_rn(b, q.y, __fmul_rn(a, q.x))));
}
__device__ __forceinline__ float3 pre_mean(const PoseRegs &p, const float x, const float y, const float z) {   // R xyz + t
    return make_float3(pre_dot3(p.R[0], p.R[1], p.R[2], x, y, z, p.t[0]), pre_dot3(p.R[3], p.R[4], p.R[5], x, y, z, p.t[1]),
                       pre_dot3(p.R[6], p.R[7], p.R[8], x, y, z, p.t[2]));
}
__device__ __forceinline__ float4 pre_rot(const PoseRegs &p, const float4 q) {   // Lq rot (quaternion product with the pose: linear in rot)
    return make_float4(pre_dot4(p.L[0], p.L[1], p.L[2], p.L[3], q), pre_dot4(p.L[4], p.L[5], p.L[6], p.L[7], q),
                       pre_dot4(p.L[8], p.L[9], p.L[10], p.L[11], q), pre_dot4(p.L[12], p.L[13], p.L[14], p.L[15], q));
}
__device__ __forceinline__ float pre_scale(const float s) { return expf(s); }
__device__ __forceinline__ float pre_opacity(const float raw, const float conf) {   // sigmoid(raw) conf
    const float s = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-raw)));
    return __fmul_rn(s, conf);
}

// The forward's inputs of Gaussian i, once for every per-Gaussian kernel of the rasterizer (preprocess_kernel and, to redo the forward's
// arithmetic on the same bits, preprocess_backward_kernel and focal_grad_kernel): the camera-frame mean, either cov3D (HAS_COV) or scale +
// quaternion and, with OPACITY, the opacity before the antialiasing factor — from the raw parameters and the pose when the caller gave those
// (pre.xyz != null, uniform; never with HAS_COV; `force_pre`: the chained backward, which has nothing else), from the camera-frame tensors
// otherwise.  What a case does not give stays as it was.
// `raw`: the raw parameters as loaded (the chained backward keeps them for its chain rule; o, c, ci with OPACITY); the first case only.
// `more_loads`: called in the first case between the raw loads and the pose arithmetic — the chained backward requests its Adam moments
// there, in the same trip to memory, where that kernel always requested them (docs/ledger.md (cm)).
struct RawGeometry {
    float x, y, z, s0, s1, s2, o, c;
    float4 q;
    long long ci;   // the Gaussian's position in conf_flat
};
template <bool HAS_COV, bool OPACITY, class MoreLoads>
__device__ __forceinline__ void load_forward_inputs(const PreXform &pre, const bool force_pre, const float *means3D,
                                                    const float *scales, const float *rotations,
                                                    const float *opacities, const float *cov3D_precomp, const int i,
                                                    float3 &mean, float3 &sc, float4 &q, float (&c3)[6], float &op, RawGeometry &raw,
                                                    MoreLoads more_loads) {
    if (!HAS_COV && (force_pre || pre.xyz != nullptr)) {   // (uniform) the pose pre-transform on the way in: the bits of pretransform_forward_kernel
        PoseRegs pose;
        load_pose(pre.Rm, pre.tv, pre.Lq, pose);
        const float rx = pre.xyz[3 * i], ry = pre.xyz[3 * i + 1], rz = pre.xyz[3 * i + 2];
        const float4 rq = reinterpret_cast<const float4 *>(pre.rot)[i];
        const float r0 = pre.scaling[3 * i], r1 = pre.scaling[3 * i + 1], r2 = pre.scaling[3 * i + 2];
        raw.x = rx; raw.y = ry; raw.z = rz; raw.q = rq; raw.s0 = r0; raw.s1 = r1; raw.s2 = r2;
        if constexpr (OPACITY) {
            raw.o = pre.opacity_raw[i];
            raw.ci = pre.mask_index ? (long long)pre.mask_index[i] : (long long)i;
            raw.c = pre.conf_flat[raw.ci];
        }
        more_loads();
        mean = pre_mean(pose, rx, ry, rz);
        q = pre_rot(pose, rq);
        sc = make_float3(pre_scale(r0), pre_scale(r1), pre_scale(r2));
        if constexpr (OPACITY) op = pre_opacity(raw.o, raw.c);
    } else {
        mean = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
        if constexpr (OPACITY) op = opacities[i];
        if (HAS_COV) {
#pragma unroll
            for (int j = 0; j < 6; j++) c3[j] = cov3D_precomp[6 * i + j];
        } else {
            sc = make_float3(scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]);
            q = reinterpret_cast<const float4 *>(rotations)[i];
        }
    }
}
template <bool HAS_COV, bool OPACITY>
__device__ __forceinline__ void load_forward_inputs(const PreXform &pre, const bool force_pre, const float *means3D,
                                                    const float *scales, const float *rotations,
                                                    const float *opacities, const float *cov3D_precomp, const int i,
                                                    float3 &mean, float3 &sc, float4 &q, float (&c3)[6], float &op, RawGeometry &raw) {
    load_forward_inputs<HAS_COV, OPACITY>(pre, force_pre, means3D, scales, rotations, opacities, cov3D_precomp, i, mean, sc, q, c3, op, raw, [] {});
}
// ... the opacity alone, for a kernel that wants it late (the same case distinction)
template <bool HAS_COV>
__device__ __forceinline__ float load_opacity_input(const PreXform &pre, const float *opacities, const int i) {
    if (!HAS_COV && pre.xyz != nullptr) return pre_opacity(pre.opacity_raw[i], pre.conf_flat[pre.mask_index ? pre.mask_index[i] : (int64_t)i]);
    return opacities[i];
}
#endif

}  // namespace das3r
