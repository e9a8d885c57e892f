/*
 * das3r_raster.h — C-ABI of libdas3r_hip.so: the MI355X (gfx950) differentiable Gaussian-splat
 * rasterizer + distCUDA2 that sit behind DAS3R's gaussian_renderer.render().
 *
 * Each entry point replaces one function of the reference's native extension modules (both are
 * un-vendored submodules of /root/reference — .gitmodules:1-6 — so the interfaces are cited by their
 * reference CALL SITES plus the upstream symbol they stand for):
 *
 *   das3r_raster_forward    <- diff_gaussian_rasterization._C.rasterize_gaussians
 *                              (upstream:rasterize_points.cu RasterizeGaussiansCUDA), reached from
 *                              /root/reference/gaussian_renderer/__init__.py:131-140 through
 *                              GaussianRasterizer.forward / _RasterizeGaussians.forward
 *   das3r_raster_backward   <- diff_gaussian_rasterization._C.rasterize_gaussians_backward
 *                              (upstream:rasterize_points.cu RasterizeGaussiansBackwardCUDA), reached from
 *                              loss.backward() at /root/reference/train_gui.py:579
 *   das3r_mark_visible      <- diff_gaussian_rasterization._C.mark_visible (GaussianRasterizer.markVisible)
 *   das3r_knn3_mean_dist2   <- simple_knn._C.distCUDA2, /root/reference/scene/gaussian_model.py:213,641
 *
 * Conventions: every data pointer is a DEVICE pointer to contiguous row-major fp32 unless
 * stated; matrices are in the reference's row-vector layout (p_row @ M, i.e. what
 * scene/cameras.py:90-93 stores); no exceptions cross the ABI — functions return >= 0 on success and a
 * negative das3r_status on failure, with a message available from das3r_last_error().  The library owns no
 * memory across calls: scratch comes from caller-supplied allocators (mirroring upstream's
 * std::function<char*(size_t)> resize callbacks) and stays alive in the caller's autograd context until
 * backward.  All work is enqueued on the caller's HIP stream.
 *
 * Deviations from the design-target ABI of SURVEY.md §8b, on purpose:
 *   - NO `_cpu` twins of the entry points.  The survey's table lists CPU variants next to the device ones; here the CPU
 *     side of every comparison is the oracle (oracle/raster_oracle.c, oracle/knn_oracle.c: test infrastructure, also the
 *     reported `cpu_baseline`), and the product has no CPU path at all — a missing GPU / library / device tensor is an
 *     error, never a fallback.  A `_cpu` twin inside this library would be exactly the fallback the parity rules forbid.
 *   - das3r_raster_forward returns the instance count as int64 and fills a `saved` record (num_rendered, capacity, the
 *     self-check ticket) instead of upstream's tuple; `capacity_hint` lets a caller forbid the speculative buffer layout;
 *     the k-NN entry point takes a caller-owned workspace.
 *
 * State between calls: the library owns no tensor and no scratch.  Per host thread, device and caller stream it keeps one non-blocking side
 * stream and two events: a training forward of SH degree >= 2 on a large scene evaluates its colours there, beside the binning kernels, and has the
 * caller's stream wait for them before it returns control of that stream (das3r_split_colour_rule).  Per host thread and per device it keeps a pinned
 * host mailbox (instance count, error word, a ring of 16 self-check tickets), the arrival counters of the count reduction,
 * the control ring of the fused scan and the last shape's instance counts (speculative capacity).  Calls of one thread on
 * one device must be issued in stream order; different threads / devices are independent.  Experiment switches (DAS3R_*
 * environment variables) are read once and cached; das3r_reload_switches() re-reads them.
 */
#ifndef DAS3R_RASTER_H
#define DAS3R_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAS3R_ABI_VERSION 16

typedef enum {
    DAS3R_OK = 0,
    DAS3R_ERR_INVALID_ARG = -1,
    DAS3R_ERR_HIP = -2,
    DAS3R_ERR_ALLOC = -3,
    DAS3R_ERR_OVERFLOW = -4
} das3r_status;

/* hipStream_t passed as an opaque pointer so that this header needs no HIP include. */
typedef void *das3r_stream_t;

/* Scratch allocator: must return a device pointer to at least `bytes` bytes, 256-byte aligned, valid until
 * the caller drops it (the caller keeps geom/binning/img alive for backward).  NULL = failure. */
typedef char *(*das3r_alloc_fn)(void *user, size_t bytes);

/* The 12 fields of GaussianRasterizationSettings (/root/reference/gaussian_renderer/__init__.py:62-78)
 * plus the tensor extents. */
typedef struct {
    int32_t P;              /* number of Gaussians */
    int32_t sh_degree;      /* active SH degree D (0..3) */
    int32_t M;              /* stored SH coefficients per channel (max_degree+1)^2; 0 if shs == NULL */
    int32_t image_width;
    int32_t image_height;
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    const float *bg;         /* [3]    device */
    const float *viewmatrix; /* [4,4]  device, row-vector layout */
    const float *projmatrix; /* [4,4]  device, row-vector layout */
    const float *campos;     /* [3]    device */
    int32_t prefiltered;     /* !=0: the caller's promise that no Gaussian fails the near-plane cull (upstream:auxiliary.h in_frustum traps
                              * when one does); das3r_raster_forward then fails with upstream's message instead of rendering */
    int32_t debug;           /* !=0: synchronise + check after every kernel */
    int64_t capacity_hint;   /* 0: the library lays the binning buffer out as it sees fit — exactly for num_rendered (which reaches
                              * the host from the first kernel of the forward), or, for a shape it has seen before, with headroom
                              * over that forward's count so that nothing waits for the count (das3r_raster_saved.capacity tells
                              * which; a scene that outgrew the headroom is redone exactly).  -1: always exactly.  Other values
                              * are reserved. */
} das3r_raster_args;

/* ABI 14, SURVEY.md section 8(f)-1: the raw parameters of a DAS3R model and the pose of the view — what das3r_pretransform_forward (below)
 * turns into camera-frame tensors in a pass of its own (/root/reference/gaussian_renderer/__init__.py:83-97,107).  Handed to the rasterizer
 * through das3r_raster_in.pre instead, the per-Gaussian kernels of forward AND backward take the transform on their way in (the same
 * arithmetic bit for bit: csrc/pretransform_math.h): means3D / rotations / scales / opacities are never written to or read from memory.
 * The backward still returns dL/d(camera-frame means3D, scales, rotations, opacities): das3r_pretransform_backward[_adam] consumes them. */
typedef struct {
    const float *xyz;            /* [P,3] */
    const float *rot;            /* [P,4] */
    const float *scaling;        /* [P,3] log scales */
    const float *opacity_raw;    /* [P,1] logits */
    const float *conf_flat;      /* confidence map, flattened */
    const int64_t *mask_index;   /* [P] position of Gaussian i in conf_flat, or NULL = identity */
    const float *R, *t, *Lq;     /* [3,3], [3], [4,4] row-major (das3r_pose_matrices[_qt]) */
} das3r_pretransform;

/* Inputs of GaussianRasterizer.forward.  Exactly one of shs/colors_precomp and exactly one of
 * (scales,rotations)/cov3D_precomp is non-NULL — unless `pre` is given: then means3D, opacities, scales and rotations are ignored
 * (may be NULL) and cov3D_precomp must be NULL. */
typedef struct {
    const float *means3D;        /* [P,3] */
    const float *opacities;      /* [P,1] */
    const float *shs;            /* [P,M,3] or NULL */
    const float *colors_precomp; /* [P,3]   or NULL */
    const float *scales;         /* [P,3]   or NULL (already activated) */
    const float *rotations;      /* [P,4]   or NULL (w,x,y,z), NOT normalised */
    const float *cov3D_precomp;  /* [P,6]   or NULL */
    const das3r_pretransform *pre; /* ABI 14: NULL, or the raw parameters + pose (HOST struct of device pointers) */
} das3r_raster_in;

typedef struct {
    float *out_color; /* [3,H,W] planar */
    int32_t *radii;   /* [P] */
    float *out_invdepth; /* ABI 16: [H,W] or NULL.  The inverse-depth image of upstream's newer rasterizer: per pixel sum_i (1/z_i) alpha_i T_i
                          * over the splats the colour is blended from (same order, same alpha / T cut-offs; z_i = view-space depth), no
                          * background term — an empty pixel is 0.  The colour, radii and everything saved for the backward pass are the
                          * same bit for bit as without it; das3r_raster_saved.flags bit 1 marks such a forward (its binning buffer is
                          * larger: it also holds the inverse depth at the bucket boundaries of long lists), and das3r_raster_backward_depth
                          * differentiates it.  DAS3R_RENDER=slices has no form of it: the forward then fails with DAS3R_ERR_INVALID_ARG
                          * before it launches anything.  NULL: as ABI 15 (a caller that zero-fills the struct keeps working). */
} das3r_raster_out;

/* What forward leaves behind for backward (upstream: geomBuffer, binningBuffer, imgBuffer, num_rendered). */
typedef struct {
    char *geom;
    char *binning;
    char *img;
    int64_t num_rendered;
    int64_t capacity;        /* instances the binning buffer was laid out for (>= num_rendered) */
    void *check_word;        /* HOST address of the {flags, tag} word this forward's binning self-check is delivered to ... */
    uint32_t check_tag;      /* ... and the tag that marks it as this forward's (0: nothing to check) */
    uint32_t flags;          /* ABI 14 (in what was the struct's tail padding: size and offsets unchanged).  Bit 0: this forward's tile lists are
                              * long and spatially coherent or skewed (a real sequence's depth maps) — it was composited by the 2x2-region kernel
                              * and its backward pass takes the 2x2-region kernel too (render_regions.hip / render_bwd_rgn.hip).  A caller that
                              * rebuilds this struct for the backward call hands the forward's value back; 0 is always valid (block walk) for
                              * das3r_raster_backward.  Bit 1 (ABI 16): the forward was given out_invdepth (das3r_raster_backward_depth needs it).
                              * Bit 2: the forward had SH coefficients at an active degree >= 2 and left the colour's Jacobian w.r.t. the view
                              * direction in geom (36 bytes per Gaussian more); the backward then reads it instead of the SH rows.  Without it
                              * (flags = 0) the backward reads the rows: the gradients are the same bit for bit either way.
                              * On the way IN, das3r_raster_forward reads bit 3 before it clears the struct: set, it is the caller's word that no
                              * backward pass will follow (an evaluation render), and the forward does not write the Jacobian (bit 2 stays clear;
                              * a backward would still be correct, reading the rows).  A zero-filled struct: the Jacobian is written as above.
                              * Bit 4, read on the way IN as bit 3 is and set again on the way out: an antialiased forward (upstream's 2D mip
                              * filter): every splat is blended with opacity o * sqrt(max(rho, 2.5e-5)), rho = det(cov2D) / det(cov2D + 0.3 I);
                              * radii, conics and colours are unchanged.  das3r_raster_backward / _depth differentiate the factor iff bit 4 is
                              * set in the flags handed back: a caller that asked for antialiasing hands the forward's flags back.  flags = 0
                              * stays valid for every forward that was not antialiased. */
} das3r_raster_saved;

/* Gradient outputs of backward.  Every buffer is fully written by the call (no pre-zeroing needed). */
typedef struct {
    float *dL_dmeans2D;        /* [P,3]  (x,y) = pixel-space grad * (W/2, H/2); z = 0 */
    float *dL_dopacities;      /* [P,1] */
    float *dL_dmeans3D;        /* [P,3] */
    float *dL_dshs;            /* [P,M,3] dense; NULL when colors_precomp was used */
    float *dL_dcolors_precomp; /* [P,3]; NULL when shs was used */
    float *dL_dscales;         /* [P,3]; NULL when cov3D_precomp was used */
    float *dL_drotations;      /* [P,4]; NULL when cov3D_precomp was used */
    float *dL_dcov3D;          /* [P,6]; NULL unless cov3D_precomp was used */
    float *scratch;            /* das3r_raster_backward_scratch_bytes(saved->capacity) bytes of caller-provided scratch: partial
                                * sums per instance (the compositing kernels use no atomics) */
    const struct das3r_chain_s *chain; /* ABI 14: NULL, or "go on through the pose pre-transform" (das3r_chain below) */
} das3r_raster_grads;

/* Returns num_rendered (>= 0) or a negative das3r_status.  Fills *saved. */
int64_t das3r_raster_forward(const das3r_raster_args *args, const das3r_raster_in *in, const das3r_raster_out *out,
                             das3r_alloc_fn alloc_geom, das3r_alloc_fn alloc_binning, das3r_alloc_fn alloc_img,
                             void *alloc_user, das3r_raster_saved *saved, das3r_stream_t stream);

int das3r_raster_backward(const das3r_raster_args *args, const das3r_raster_in *in, const das3r_raster_saved *saved,
                          const float *dL_dpix /* [3,H,W] */, const das3r_raster_grads *grads, das3r_stream_t stream);

/* Bytes of device scratch das3r_raster_backward needs in grads->scratch for a forward with the given saved->capacity:
 * 36 bytes (nine partial sums) per instance + 16 (the rows are read back as 16-byte words).  16-byte alignment of the buffer
 * lets the per-Gaussian backward do that; any other alignment falls back to 4-byte loads. */
size_t das3r_raster_backward_scratch_bytes(int64_t capacity);

/* ABI 16: the backward of a forward that was given out_invdepth — das3r_raster_backward for the colour gradient dL_dpix [3,H,W] plus
 * that of dL_dinvdepth [H,W] (either may be all zero), into the same gradient outputs (grads->chain included: the depth term reaches
 * dL/dmeans3D before the chain carries it on).  grads->scratch: das3r_raster_backward_depth_scratch_bytes(saved->capacity) bytes.
 * A saved state without flags bit 1 (a colour-only forward, or a caller that handed back flags = 0) is refused with
 * DAS3R_ERR_INVALID_ARG before anything is launched, as are DAS3R_RENDER_BWD=scan* (and the experiments build's mfma / stream). */
int das3r_raster_backward_depth(const das3r_raster_args *args, const das3r_raster_in *in, const das3r_raster_saved *saved,
                                const float *dL_dpix /* [3,H,W] */, const float *dL_dinvdepth /* [H,W] */, const das3r_raster_grads *grads,
                                das3r_stream_t stream);
/* das3r_raster_backward_scratch_bytes' nine-float rows twice (256-byte aligned between): the colour pass's and the depth pass's, whose
 * first column is the per-instance sum over pixels of alpha T dL/dinvdepth. */
size_t das3r_raster_backward_depth_scratch_bytes(int64_t capacity);

/* Additive under ABI 16: a backward pass that also returns the gradient of its loss with respect to two log-focal offsets s = (s_x, s_y).
 * The forward at s is the forward with tanfovx e^(-s_x), tanfovy e^(-s_y) and the clip-x / clip-y columns of projmatrix (elements 4r and
 * 4r + 1) scaled by e^(s_x) / e^(s_y); sums[0 .. 1] = dL/ds at s = 0 for L = <dL_dpix, colour> (+ <dL_dinvdepth, inverse depth>), every
 * discrete decision of the forward held fixed (cull, radius, tile rectangle, lists, the 1/255 and T < 1e-4 cut-offs, the EWA clamp flags; a
 * clamped ray is a constant, as it is for dL/dmeans3D).  With s_x = -log tan(FoVx / 2): dL/dFoVx = -sums[0] / sin(FoVx).
 * It is the whole backward: with dL_dinvdepth == NULL das3r_raster_backward, otherwise das3r_raster_backward_depth — the same launches, the
 * same gradient tensors bit for bit, grads->scratch sized by the matching *_scratch_bytes — with one per-Gaussian kernel and its one-workgroup
 * finish in front of the per-Gaussian backward (with grads->chain: before the Adam step touches the parameters).
 * per_splat ([P,2] or NULL): every splat's own contribution, exact zeros for a splat that reached no tile; sums is their sum in a fixed order
 * (no float atomics: bit-identical from run to run).  workspace: das3r_raster_focal_workspace_bytes(P) bytes, 4-byte aligned.  Neither sums,
 * per_splat nor workspace needs initialising.  P == 0 or nothing rendered: sums = 0, per_splat = 0.
 * NULL sums / workspace, and with dL_dinvdepth whatever das3r_raster_backward_depth refuses: DAS3R_ERR_INVALID_ARG before anything is launched. */
size_t das3r_raster_focal_workspace_bytes(int32_t P);
int das3r_raster_backward_focal(const das3r_raster_args *args, const das3r_raster_in *in, const das3r_raster_saved *saved,
                                const float *dL_dpix /* [3,H,W] */, const float *dL_dinvdepth /* [H,W], or NULL: colour only */,
                                const das3r_raster_grads *grads, float *sums /* [2] */, float *per_splat /* [P,2] or NULL */, float *workspace,
                                das3r_stream_t stream);

/* das3r_raster_forward returns as soon as its kernels are enqueued.  Its binning kernels check themselves (a bounded wait on
 * another workgroup that timed out, an index out of range, counts that do not add up) and leave one word for the host; this call
 * waits (bounded) for that word of the forward that produced `saved` and returns DAS3R_ERR_HIP if the forward's image and lists are
 * invalid.  das3r_raster_backward calls it before launching anything; callers that render without a backward (evaluation) call it
 * before they use the image.  A forward with args->debug != 0 has already waited for it.  The ticket may be examined from any
 * host thread. */
int das3r_raster_check(const das3r_raster_saved *saved, das3r_stream_t stream);

/* present[i] = (view-space z of means3D[i]) > near plane (0.001, /root/reference/README.md:41-44). */
int das3r_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                       uint8_t *present, das3r_stream_t stream);

/* distCUDA2: out[i] = mean of squared distances to the 3 nearest other points.  `workspace` must hold
 * das3r_knn3_workspace_bytes(P) bytes of device memory. */
size_t das3r_knn3_workspace_bytes(int32_t P);
int das3r_knn3_mean_dist2(int32_t P, const float *points /* [P,3] */, float *out /* [P] */, char *workspace,
                          das3r_stream_t stream);

/* ---- opt-in fused callers' work around the rasterizer (the default DAS3R path does not need them) ---- */

/* pose (qw,qx,qy,qz,tx,ty,tz) -> mats[28] = R (9, rotation of the normalised quaternion: get_camera_from_tensor), t (3), Lq (16,
 * left-multiplication matrix of the raw quaternion: quadmultiply) — the three small matrices das3r_pretransform_* take — and
 * the chain rule back from dL/d(mats) (the g_small of das3r_pretransform_backward) to dL/d(pose). */
int das3r_pose_matrices(const float *pose, float *mats, das3r_stream_t stream);
int das3r_pose_chain(const float *pose, const float *g_mats, float *g_pose, das3r_stream_t stream);
/* The same two with the pose given as DAS3R stores it — one row of Q (frames, 4) and one of T (frames, 3), scene/gaussian_model.py:
 * 149-184 — and its gradient written straight into the rows of two dense gradient buffers (no torch.cat, no index backward).
 * das3r_pose_chain_qt also leaves g_mats[0 .. 28) ZERO: the sums of das3r_pretransform_backward are accumulated into it, so a
 * caller-owned buffer stays zero at rest (ABI 10). */
int das3r_pose_matrices_qt(const float *q, const float *t, float *mats, das3r_stream_t stream);
int das3r_pose_chain_qt(const float *q, float *g_mats, float *g_q, float *g_t, das3r_stream_t stream);
/* ABI 15 — das3r_pose_chain_qt that first ZEROES the rows zero_q[0 .. 4) / zero_t[0 .. 3) (either may be NULL; they may be g_q / g_t
 * themselves): the rows the previous view left in dense (frames, 4) / (frames, 3) gradient buffers, which the camera optimizer (dense
 * Adam over every frame, train_gui.py:584-586) must find zero — two fill launches per iteration otherwise. */
int das3r_pose_chain_qt_rearm(const float *q, float *g_mats, float *g_q, float *g_t, float *zero_q, float *zero_t, das3r_stream_t stream);
/* §8f-1: the per-Gaussian pre-transform + activations of /root/reference/gaussian_renderer/__init__.py:83-97,107 in one
 * pass: means3D = R xyz + t, rotations = Lq rot (quadmultiply(pose[:4], .) as a 4x4 matrix), scales = exp(scaling),
 * opacities = sigmoid(opacity_raw) * conf_flat[mask_index[i]] (mask_index NULL = identity).  R [3,3], t [3], Lq [4,4]:
 * row-major device tensors.  backward: g_conf_flat (size of conf_flat) and g_small [28] = dL/dR (9), dL/dt (3),
 * dL/dLq (16) must be zero on entry. */
int das3r_pretransform_forward(int32_t P, const float *xyz, const float *rot, const float *scaling, const float *opacity_raw,
                               const float *conf_flat, const int64_t *mask_index, const float *R, const float *t, const float *Lq,
                               float *means3D, float *rotations, float *scales, float *opacities, das3r_stream_t stream);
int das3r_pretransform_backward(int32_t P, const float *xyz, const float *rot, const float *scaling, const float *opacity_raw,
                                const float *conf_flat, const int64_t *mask_index, const float *R, const float *Lq,
                                const float *g_means3D, const float *g_rot, const float *g_scales, const float *g_opac, float *g_xyz,
                                float *g_rotation, float *g_scaling, float *g_opacity_raw, float *g_conf_flat, float *g_small,
                                das3r_stream_t stream);

/* §8f-2: one multi-tensor Adam step (torch.optim.Adam semantics, no weight decay / amsgrad;
 * /root/reference/scene/gaussian_model.py:236-261).  A tensor is `rows` rows of `row_len` floats of which only the first
 * `active_len` are updated (degree-aware SH coefficients; active_len == row_len for ordinary tensors).  The first `head_len`
 * floats of a row may use a different learning rate (one [P,16,3] SH tensor whose DC part and rest part belong to the
 * reference's two parameter groups f_dc / f_rest): they step with step_size, the others with step_size_tail; head_len == 0 or
 * >= active_len means one rate (step_size) for the whole row.  `tensors` is a HOST array. */
typedef struct {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t rows;
    int32_t row_len;
    int32_t active_len;
    float step_size;  /* lr / (1 - beta1^t) */
    float bc2_sqrt;   /* sqrt(1 - beta2^t) */
    int32_t head_len;
    float step_size_tail;
    int32_t grad_row_len; /* ABI 9: floats per row of `grad` when it is more compact than the parameter (>= active_len: e.g. the
                             gradient of the first 3 of 15 SH coefficients as [P, 3, 3]); 0 = row_len */
    int32_t state_row_len; /* ABI 14 (in what was tail padding): floats per row of exp_avg / exp_avg_sq when the MOMENTS are kept more
                              compact than the parameter (>= active_len; 0 = row_len).  The moments of SH coefficients above the active
                              degree are exactly zero: FusedAdam keeps only the active prefix — at degree 1, [P, 3, 3] beside a [P, 15, 3]
                              parameter — so that four of the step's six streams are dense (adam_kernel 0.46 -> see docs/ledger.md (bh)) */
    float *mirror;          /* ABI 14: NULL, or a second place the UPDATED active values of each row are written to: row r, column c of the active
                               prefix -> mirror[r * mirror_row_len + c].  das3r_amd/fast_step.py keeps the packed [P, K, 3] SH tensor the rasterizer
                               reads (DC + the active rest coefficients) current this way — the steps of f_dc and f_rest write into it, at column
                               offsets 0 and 3 — instead of concatenating the two parameters before every render (0.16 ms at 2.13 M Gaussians) */
    int32_t mirror_row_len;
} das3r_adam_tensor;
int das3r_adam_step(int32_t n, const das3r_adam_tensor *tensors, float beta1, float beta2, float eps, das3r_stream_t stream);
/* The same step taken iff the DEVICE scalar gate[0] > threshold (DAS3R's camera optimizer steps only when the frame PSNR exceeds
 * 26 dB, train_gui.py:584-586; deciding on the host stalls it every iteration).  state: two device int32, zero-initialised by the
 * caller: [0] counts the steps actually taken (bias corrections are computed from it on the device), [1] is scratch.
 * tensors[i].step_size / step_size_tail hold the plain learning rates here; bc2_sqrt is ignored. */
int das3r_adam_step_gated(int32_t n, const das3r_adam_tensor *tensors, float beta1, float beta2, float eps, const float *gate,
                          float threshold, int32_t *state, das3r_stream_t stream);

/* ABI 14 — das3r_raster_grads.chain: the rasterizer's backward goes on where it used to stop.  With in->pre (raw parameters + pose) its
 * per-Gaussian kernel holds dL/d(camera-frame means, scales, rotations, opacities) in registers: instead of writing them for
 * das3r_pretransform_backward_adam to read back, it applies that function's chain rule and Adam step itself (the same arithmetic, bit for
 * bit: csrc/pretransform_chain.h) — slots[0..3] = xyz, rotation, scaling, opacity exactly as for das3r_pretransform_backward_adam (they
 * must be the tensors of in->pre), g_conf_flat written at the mask positions, the 28 pose sums ADDED to g_small (zero at rest) in a fixed
 * order.  grads->dL_dmeans3D / dL_dscales / dL_drotations / dL_dopacities are then not written (may be NULL).  SH coefficients in an
 * unstaged layout only (M < 16, or the active degree below 2): otherwise DAS3R_ERR_INVALID_ARG, use the two calls. */
typedef struct das3r_chain_s {
    float *g_conf_flat;
    float *g_small;
    const struct das3r_adam_slot_s *slots;
    float beta1, beta2, eps;
} das3r_chain;

/* ABI 11: the backward of the pre-transform with the Adam step of the four tensors it differentiates — xyz, rotation, scaling, raw
 * opacity: the reference's groups "xyz", "rotation", "scaling", "opacity" (/root/reference/scene/gaussian_model.py:236-261) — taken in the
 * same pass: their gradients are neither written nor read back, the parameters are read once for both.  slots[0 .. 3] (a HOST array)
 * name the four tensors in that order (they are the xyz / rot / scaling / opacity_raw of das3r_pretransform_backward, updated in
 * place) with their moments and step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) as in das3r_adam_tensor.  g_conf_flat and
 * g_small leave as from das3r_pretransform_backward (zero on entry): the confidence map and the camera pose have their own steps.
 * Same arithmetic as das3r_pretransform_backward followed by das3r_adam_step on the four tensors. */
typedef struct das3r_adam_slot_s {
    float *param, *exp_avg, *exp_avg_sq;
    float step_size, bc2_sqrt;
} das3r_adam_slot;
int das3r_pretransform_backward_adam(int32_t P, const float *conf_flat, const int64_t *mask_index, const float *R, const float *Lq,
                                     const float *g_means3D, const float *g_rot, const float *g_scales, const float *g_opac,
                                     float *g_conf_flat, float *g_small, const das3r_adam_slot *slots, float beta1, float beta2, float eps,
                                     das3r_stream_t stream);
/* ABI 11: g_small of das3r_pretransform_backward alone — for a pass that differentiates nothing but the camera pose (the held-out
 * pose alignment of /root/reference/train_test_psnr.py). */
int das3r_pretransform_pose_sums(int32_t P, const float *xyz, const float *rot, const float *R, const float *Lq, const float *g_means3D,
                                 const float *g_rot, float *g_small, das3r_stream_t stream);

/* ---- fused photometric loss (opt-in) ------------------------------------------------------------------
 * DAS3R's per-iteration loss (/root/reference/train_gui.py:560-571, utils/loss_utils.py:39-66): with image = render * static,
 * gt' = gt * static:  loss = mean[(1 - lambda) |image - gt'| + lambda (1 - SSIM_map(image, gt'))] over all 3*H*W elements.
 * forward: every 16x16 tile writes partials[tile][8] = {sum |d|, sum (1 - ssim), sum d^2 for channels 0, 1, 2, -, -, -}
 * (the caller adds the das3r_photometric_blocks(H, W) rows: loss = ((1-lambda) S0 + lambda S1) / (3HW), mse_c = S(2+c) / (HW))
 * and the derivative maps dmaps[4][3][H][W] the backward consumes.  backward: d_render[3,H,W], d_static[H,W] for the device
 * scalar grad_loss = dL/dloss.  render/gt are [3,H,W], static_mask [H,W], all fp32 device pointers. */
int64_t das3r_photometric_blocks(int32_t H, int32_t W);
int das3r_photometric_forward(int32_t H, int32_t W, const float *render, const float *gt, const float *static_mask, float lambda,
                              float *partials, float *dmaps, das3r_stream_t stream);
/* Adds the das3r_photometric_blocks(H, W) rows of `partials` on the device: out8 = {loss, mse_r, mse_g, mse_b, psnr_frame, 0, 0, 0}
 * with psnr_frame = mean_c 20 log10(1 / sqrt(mse_c)) (utils/image_utils.py:17-19; the 26 dB gate of train_gui.py:584) — one launch
 * instead of a dozen scalar PyTorch kernels per iteration (ABI 10). */
int das3r_photometric_finish(int32_t H, int32_t W, const float *partials, float lambda, float *out8, das3r_stream_t stream);
int das3r_photometric_backward(int32_t H, int32_t W, const float *render, const float *gt, const float *static_mask, float lambda,
                               const float *dmaps, const float *grad_loss, float *d_render, float *d_static, das3r_stream_t stream);
/* ABI 15 — das3r_photometric_backward and das3r_photometric_finish as ONE launch: the first workgroup of the backward kernel adds the
 * forward's tile sums (`partials`) into out8 on its way in.  Same values, bit for bit; one launch less between the two rasterizer passes. */
/* ABI 15 — the SSIM map itself (utils/loss_utils.py:39-66, size_average = False: 11 x 11 Gaussian window, sigma 1.5, zero padding, per channel)
 * of two [3, H, W] images, and its backward for an arbitrary upstream gradient [3, H, W] — for callers that compose the loss themselves
 * (train_gui.py:566-571 combines the map with its L1 map).  dmaps [4][3][H][W] and partials [das3r_photometric_blocks][8] are scratch the
 * forward fills (the backward reads dmaps). */
int das3r_ssim_map_forward(int32_t H, int32_t W, const float *img1, const float *img2, float *ssim_map, float *dmaps, float *partials,
                           das3r_stream_t stream);
int das3r_ssim_map_backward(int32_t H, int32_t W, const float *img1, const float *img2, const float *dmaps, const float *grad_map,
                            float *d_img1, float *d_img2, das3r_stream_t stream);
int das3r_photometric_backward_finish(int32_t H, int32_t W, const float *render, const float *gt, const float *static_mask, float lambda,
                                      const float *dmaps, const float *grad_loss, float *d_render, float *d_static, const float *partials,
                                      float *out8, das3r_stream_t stream);

/* ---- per-frame exposure compensation in the photometric loss (opt-in) ----------------------------------------------------
 * Additive symbols under ABI 16.  `exposure` is a DEVICE pointer to one view's 3 x 4 row-major matrix E (upstream 3DGS's convention); with
 *     comp_c(p) = sum_i render_i(p) E[i][c] + E[c][3]
 * the loss, the MSEs, psnr_frame and d_static above are those of comp in the render's place; E = [I | 0] gives the values of the entry
 * points without exposure bit for bit.  With g_c = dL/d image_c:
 *     d_render_i(p) = static(p) sum_c E[i][c] g_c(p)          d_static(p) = sum_c (g_c comp_c + db_c gt_c)
 *     dL/dE[i][c]   = sum_p g_c(p) static(p) render_i(p)      dL/dE[c][3] = sum_p g_c(p) static(p)
 * das3r_photometric_backward_finish_exposure writes every tile's twelve sums to epartials[das3r_photometric_blocks(H, W)][16] (scratch; NULL:
 * no exposure gradient is taken); partials / out8 as in das3r_photometric_backward_finish, or both NULL for no loss reduction.
 * das3r_exposure_grad_finish: one workgroup zeroes zero_row[12] (NULL: nothing; may be grad_row) and then writes the rows of epartials, added
 * in a fixed order, to grad_row[12] — row `uid` of a dense [n_train, 3, 4] gradient that is zero elsewhere.  No floating-point atomics:
 * bit-identical from run to run.  A NULL `exposure` (the entry points above are the form without) or any other bad argument:
 * DAS3R_ERR_INVALID_ARG with a das3r_last_error() message, nothing launched. */
int das3r_photometric_forward_exposure(int32_t H, int32_t W, const float *render, const float *gt, const float *static_mask, float lambda,
                                       const float *exposure, float *partials, float *dmaps, das3r_stream_t stream);
int das3r_photometric_backward_finish_exposure(int32_t H, int32_t W, const float *render, const float *gt, const float *static_mask, float lambda,
                                               const float *exposure, const float *dmaps, const float *grad_loss, float *d_render,
                                               float *d_static, const float *partials, float *out8, float *epartials, das3r_stream_t stream);
int das3r_exposure_grad_finish(int32_t H, int32_t W, const float *epartials, float *grad_row, float *zero_row, das3r_stream_t stream);

/* ---- inverse-depth L1 term (depth-supervised training; opt-in) ------------------------------------------------------------
 * Additive symbols under ABI 16 (no struct and no existing entry point changes, as antialiasing and the split-colour rule were added).
 * With D = the rasterizer's inverse-depth image (das3r_raster_out.out_invdepth), D* = target, m = mask, s = static_mask (NULL = 1; taken as
 * a constant: no gradient to it), all [H,W] fp32 device pointers:
 *     L_pure     = mean over all H*W pixels of |(D - D*) m s|
 *     d_invdepth = grad_loss * weight * m s sgn((D - D*) m s) / (H W)      [H,W]; grad_loss: device scalar, NULL = 1; sgn(0) = 0
 * A pixel with m s == 0 gives exactly 0 to both, whatever D* holds there (NaN included).  Values go into the caller's out8 in stream
 * order: out8[5] = L_pure, out8[6] = weight * L_pure, out8[0] += weight * L_pure — behind das3r_photometric_backward_finish that makes
 * out8[0] the step's total loss; a stand-alone caller hands in a zeroed out8.  partials: scratch of das3r_depth_l1_blocks(H, W) rows of 8
 * floats (one partial sum per workgroup; need not be zeroed).  Two launches: the sweep, then one workgroup that adds the rows in index order
 * — no floating-point atomics, bit-identical from run to run.  H <= 0, W <= 0, H * W > 2^30 or a NULL pointer other than static_mask /
 * grad_loss: DAS3R_ERR_INVALID_ARG with a das3r_last_error() message, nothing launched. */
int64_t das3r_depth_l1_blocks(int32_t H, int32_t W);
int das3r_depth_l1(int32_t H, int32_t W, const float *invdepth, const float *target, const float *mask, const float *static_mask, float weight,
                   const float *grad_loss, float *d_invdepth, float *partials, float *out8, das3r_stream_t stream);

/* ---- pruning: selection and stable compaction (opt-in) ---------------------------------------------------------------------
 * Additive symbols under ABI 16.  The reference carries the operation and never calls it (scene/gaussian_model.py:436-468 prune_points /
 * _prune_optimizer, 552-566 densify_and_prune; call sites commented out, train_gui.py:612-623).
 *
 * das3r_prune_select: one decision per Gaussian.  With eff = sigmoid(opacity_raw[i]) * conf_flat[mask_index[i]] (mask_index NULL =
 * identity), computed by the helper the pre-transform hands the rasterizer its opacity with (csrc/pretransform_math.h pre_opacity: the
 * same bits), Gaussian i is DROPPED iff
 *     eff < min_opacity                                                    (a NaN compares false: kept; a negative conf: dropped)
 *  or max_world_scale > 0 and max_k exp(scaling[3 i + k]) > max_world_scale    (scaling NULL or max_world_scale <= 0: criterion off)
 *  or also_drop != NULL and also_drop[i] != 0.
 * dst_index[i] = the new row of a kept Gaussian — its rank among the kept ones, so order is preserved (depth ties are broken by Gaussian
 * index) — or -1 for a dropped one.  count: device int32 words, DAS3R_PRUNE_COUNT_WORDS(P) of them; count[0] leaves as the number of kept
 * rows, the others are scratch (per-workgroup counts; need not be zeroed).  Three launches on `stream` (flags + per-workgroup counts, a
 * one-workgroup scan of the counts, ranks): nothing is handed from workgroup to workgroup inside a launch.  P == 0: count[0] = 0.
 *
 * das3r_prune_compact: dst[dst_index[i]] = src[i] for every row i with 0 <= dst_index[i] < kept, for up to 16 row-major tensors in ONE
 * launch.  `tensors` is a HOST array.  row_bytes is a multiple of 4 (0: the tensor has no columns, nothing to move); rows are moved in
 * 16-byte units where row_bytes and both pointers allow it, else 8, else 4.  Out of place: src and dst must not overlap (a later
 * workgroup's destination could lie on an earlier one's unread source).  P * row_bytes / unit must stay below 2^32.  P == 0 or kept == 0:
 * nothing is launched. */
#define DAS3R_PRUNE_GROUP_ROWS 1024
#define DAS3R_PRUNE_COUNT_WORDS(P) (1 + ((int64_t)(P) + DAS3R_PRUNE_GROUP_ROWS - 1) / DAS3R_PRUNE_GROUP_ROWS)
typedef struct {
    const void *src; /* [P] rows */
    void *dst;       /* [kept] rows */
    int64_t row_bytes;
} das3r_prune_tensor;
int das3r_prune_select(int32_t P, const float *opacity_raw, const float *conf_flat, const int64_t *mask_index, float min_opacity,
                       const float *scaling, float max_world_scale, const uint8_t *also_drop, int32_t *dst_index, int32_t *count,
                       das3r_stream_t stream);
int das3r_prune_compact(int32_t P, int32_t kept, const int32_t *dst_index, int32_t n, const das3r_prune_tensor *tensors,
                        das3r_stream_t stream);

/* ---- voxel thinning: one Gaussian per cell of a voxel grid (opt-in) ------------------------------------------------------------
 * Additive symbols under ABI 16 (csrc/thin.hip; the same rule in torch: das3r_amd/thin.py voxel_keep_torch, which the tests hold the kernels
 * to bit for bit).  DAS3R starts with one Gaussian per confident pixel of every frame: a static surface seen in F frames is about F coincident
 * Gaussians.  das3r_thin_voxels decides which of them stay; the surgery is das3r_prune_select(also_drop) + das3r_prune_compact.
 *
 * Cell of point i:  c_k = floorf(xyz[3 i + k] * inv_edge), k = 0, 1, 2 — ONE fp32 multiply per axis, no division, no offset, nothing
 * contracted; inv_edge = fp32(1 / edge) is computed once by the host.  The point is PLACEABLE iff the three products are finite and every
 * c_k lies in [-2^20, 2^20); its key is the 63-bit pack (c_0 + 2^20) << 42 | (c_1 + 2^20) << 21 | (c_2 + 2^20).  A point that is not
 * placeable never merges with anything.
 * Winner of a cell: the placeable point with the highest score[i]; equal scores (-0 equals +0) go to the lower index; a NaN score loses
 * to every number, among NaNs the lower index wins.  score NULL: all scores equal, the lowest index of the cell wins.
 *   keep[i]   1 for a winner and for a point that is not placeable, else 0
 *   count[i]  the cell's population for a winner, 1 for a point that is not placeable, 0 for a dropped point
 *   info[0]   the number kept;  info[1]  0, or 1 when the table was exhausted (impossible at the workspace size below: load factor <= 1/2;
 *             a point that found no slot is then treated as not placeable)
 * Nothing in the result depends on launch geometry, scheduling or the hash: two runs are bit-identical.
 * workspace: das3r_thin_workspace_bytes(P) bytes, 8-byte aligned, need not be initialised: an open-addressing table of S slots, S the power
 * of two >= max(2 P, 64), 20 bytes per slot (64-bit key, 64-bit best word, 32-bit population) + 4 bytes per point = 44 - 84 bytes per point;
 * at 7.37 M points S = 2^24: 49.5 bytes per point.  Launches on `stream`: the memsets, an insert pass, a resolve pass (a thread per point
 * each; bounded probing, no thread waits for another, integer vector atomics only).  P == 0: nothing is launched, info = {0, 0}.
 * P < 0 or > 2^30 (das3r_thin_workspace_bytes: 0), a NULL pointer other than score, or inv_edge not finite or <= 0: DAS3R_ERR_INVALID_ARG with a
 * das3r_last_error() message. */
size_t das3r_thin_workspace_bytes(int32_t P);
int das3r_thin_voxels(int32_t P, const float *xyz, const float *score /* or NULL */, float inv_edge, uint8_t *keep, int32_t *count,
                      int32_t *info /* [2] */, char *workspace, das3r_stream_t stream);

/* ---- extra per-Gaussian channels over a forward's lists (opt-in) --------------------------------------------------------------
 * Additive symbols under ABI 16.  das3r_raster_aux_forward blends a caller's rows features[P][C] exactly as the forward blended its colours,
 *     out[c][pixel] = sum_k features[g_k][c] alpha_k T_k        over the splats g_k the pixel's colour was blended from (same order, same
 *                                                               alpha, same stop), no background term: an empty pixel is 0
 * and das3r_raster_aux_adjoint is its adjoint,
 *     dL_dfeat[i][c] (=, or += with accumulate != 0)  sum over pixels and the list entries of Gaussian i of  alpha T dL_dout[c][pixel];
 * with dL_dout = 1 and C = 1 that is the blending-weight mass of every Gaussian in the view.  Both read what ANY forward enqueued on the
 * stream left in `saved` (geom / binning / img, num_rendered, capacity, the self-check ticket): with or without das3r_raster_in.pre, with
 * or without out_invdepth, antialiased or not (the factor is part of the saved opacity), an evaluation forward (flags bit 3), every
 * binning path and forward kernel — any number of times while the caller keeps the three buffers, before or after
 * das3r_raster_backward / _depth (neither call writes what the other reads).  No preprocess, emission or sort is repeated.
 * THE GEOMETRY IS CONSTANT in these two calls: alpha and T are the forward's, and neither sends a gradient to means, scales, rotations or
 * opacities.  The gradients of an aux image and of the coverage image with respect to the geometry are das3r_raster_aux_backward's (below).
 * args supplies P, image_width, image_height and debug only.  1 <= C <= DAS3R_AUX_MAX_CHANNELS per call (wider tensors: several calls).
 * scratch: das3r_raster_aux_scratch_bytes(saved->capacity, C) bytes (one row of C sums per list entry; need not be zeroed).  dL_dfeat is
 * fully written (zeros for a Gaussian that was not rendered) unless accumulate.  No floating-point atomics: bit-identical from run to run.
 * A bad C or a NULL pointer: DAS3R_ERR_INVALID_ARG with a das3r_last_error() message before anything is launched; P == 0 or nothing
 * rendered: `out` is zeroed (dL_dfeat too, unless accumulate).  The forward's binning self-check is examined first (das3r_raster_check). */
#define DAS3R_AUX_MAX_CHANNELS 8
int das3r_raster_aux_forward(const das3r_raster_args *args, const das3r_raster_saved *saved, int32_t C, const float *features /* [P,C] */,
                             float *out /* [C,H,W] planar */, das3r_stream_t stream);
size_t das3r_raster_aux_scratch_bytes(int64_t capacity, int32_t C);
int das3r_raster_aux_adjoint(const das3r_raster_args *args, const das3r_raster_saved *saved, int32_t C, const float *dL_dout /* [C,H,W] */,
                             float *dL_dfeat /* [P,C] */, int32_t accumulate, float *scratch, das3r_stream_t stream);

/* ---- aux channels and coverage: gradients to the geometry (opt-in) ---------------------------------------------------------------
 * Additive symbols under ABI 16.  das3r_raster_aux_backward is the whole backward pass of
 *     L = <dL_dout, das3r_raster_aux_forward's image of `features`> + <dL_dalpha, 1 - final_T>            (either term may be absent)
 * for the forward that left `saved`, with respect to the forward's geometry inputs — and, with dL_dfeatures, to `features` as well (the sums
 * of das3r_raster_aux_adjoint, from the same walk).  Launches: ONE compositing kernel (render_aux_backward_kernel: every pixel replayed back to
 * front over the saved lists from T = final_T, stop n_contrib; no second forward, no preprocess, emission or sort), the gather for
 * dL_dfeatures if asked, and the per-Gaussian backward das3r_raster_backward ends with — the antialiasing factor of an antialiased forward
 * (flags bit 4) is differentiated exactly as for a colour loss.  Every discrete decision of the forward is held fixed: cull, radius, tile
 * rectangle, lists, the 1/255 and T < 1e-4 cut-offs, n_contrib.
 * The coverage term is differentiated in the direct form dL/dalpha_k += dL_dalpha T_final / (1 - alpha_k).  Ask for it with dL_dalpha; do NOT
 * blend a column of ones instead: the same value then comes out of T_k - R / (1 - alpha_k), which cancels in fp32 (measured on pixels
 * with hundreds of faint layers: 1.3e-4 .. 5.4e-4 of the largest gradient against 3e-6 for the direct form).
 * args / in: the ones the forward was given (the per-Gaussian backward reads the inputs), as for das3r_raster_backward.  0 <= C <=
 * DAS3R_AUX_MAX_CHANNELS; C == 0 is the coverage term alone.  features [P, C] and dL_dout [C, H, W] are required iff C > 0; dL_dalpha [H, W]
 * or NULL; dL_dfeatures [P, C] or NULL (fully written; zeros for a Gaussian that was not rendered).
 * grads: every buffer das3r_raster_backward would ask for, fully written; the colour gradient of this loss is identically zero, and
 * dL_dshs / dL_dcolors_precomp (whichever the forward's input calls for — still required) is written as zeros.  grads->scratch:
 * das3r_raster_aux_backward_scratch_bytes(saved->capacity, C) bytes — the nine-float rows, then C floats per instance — 4-byte aligned, need
 * not be initialised.  No floating-point atomics: bit-identical from run to run.  P == 0 or nothing rendered: every output is zeros.
 * DAS3R_ERR_INVALID_ARG with a das3r_last_error() message, before anything is launched: grads->chain != NULL (the chained backward is the
 * colour loss's), C outside 0 .. 8, C == 0 with NULL dL_dalpha (or with dL_dfeatures), a NULL among the pointers the chosen C needs, NULL
 * grads->scratch, and whatever das3r_raster_backward refuses.  The forward's binning self-check is examined first (das3r_raster_check).
 * One workgroup per tile: few tiles with very long lists (~10 k entries) leave most of the chip idle — see docs/ledger.md (ck). */
size_t das3r_raster_aux_backward_scratch_bytes(int64_t capacity, int32_t C);
int das3r_raster_aux_backward(const das3r_raster_args *args, const das3r_raster_in *in, const das3r_raster_saved *saved, int32_t C,
                              const float *features /* [P,C]; NULL iff C == 0 */, const float *dL_dout /* [C,H,W]; NULL iff C == 0 */,
                              const float *dL_dalpha /* [H,W] or NULL */, float *dL_dfeatures /* [P,C] or NULL */,
                              const das3r_raster_grads *grads, das3r_stream_t stream);

/* ---- ray-distortion regulariser over a forward's lists, forward and backward (opt-in) -----------------------------------------------
 * Additive symbols under ABI 16.  The distortion loss of Mip-NeRF 360 / 2DGS: the pairwise spread of the blending weights along a ray.  It is
 * quadratic in the weights, so no blend of per-Gaussian channels (das3r_raster_aux_forward) expresses it.
 * Definition.  For the forward that left `saved`, and for a pixel whose colour was blended from list entries k = 0 .. n-1:
 *   - the entries are the same ones, in the same order, with the same alpha and the same stop at n_contrib as the colour;
 *   - w_k = alpha_k T_k;
 *   - m_k = 1 / z_k, where z_k is the fp32 view-space depth the forward saved in the splat record (the staged 1/z of the inverse-depth image).
 *
 *     D[pixel] = sum_{j<k} w_j w_k (m_j - m_k)
 *              = sum_k w_k (B_{k-1} - m_k A_{k-1}),     A_k = sum_{j<=k} w_j,  B_k = sum_{j<=k} w_j m_j
 *
 *   - A tile's list is ordered by (depth, index), so every term is >= 0 and D = 1/2 sum_i sum_j w_i w_j |m_i - m_j|.
 *   - There is no background term.  An empty pixel or a pixel with one contributor is exactly 0.
 *   - Inverse depth: 2DGS's NDC depth is affine in 1/z, and out_invdepth is in inverse depth already.
 *   - D is invariant under m -> m + c.  Both kernels take m RELATIVE TO THE PIXEL'S WEIGHTED MEAN mu = B / A: the forward as a running mean,
 *     B_{k-1} - m_k A_{k-1} = A_{k-1} (mu_{k-1} - m_k) with mu_k = mu_{k-1} + w_k (m_k - mu_{k-1}) / A_k, the backward relative to the final
 *     one, where B = 0.  So B - m A does not cancel on lists whose depths nearly agree — the lists the loss exists for — and a single
 *     outlier in front (a faint splat just past the near plane) does not cost the others their bits, as a fixed first-entry reference would.
 * Backward.  With SA_k = sum_{j>k} w_j, SB_k = sum_{j>k} w_j m_j, A = sum w and B = sum w m:
 *     q_k = dD/dw_k = m_k (2 SA_k - A) - (2 SB_k - B),          dD/dm_k = w_k (2 SA_k + w_k - A),
 *     dD/dalpha_k = T_k q_k - (sum_{j>k} w_j q_j) / (1 - alpha_k)
 * — the colour recurrence on the per-pair scalar dL_ddist[pixel] q_k; SA and SB are running sums of the back-to-front replay, A = 1 - final_T.
 * THE TOTALS PLANE is the chosen design for B: das3r_raster_distortion_forward leaves the pixel's total in `totals` [H,W] (caller memory;
 * NULL: not wanted) as the mean mu = B / A — the shift in which the shifted total is zero, 0 for an empty pixel — and
 * das3r_raster_distortion_backward takes that plane back.  The backward makes no front-to-back sweep of its own.
 * Every discrete decision of the forward is held fixed, as for das3r_raster_aux_backward: cull, radius, tile rectangle, lists and their order,
 * the 1/255 and T < 1e-4 cut-offs, n_contrib.
 * Launches.  Forward: ONE kernel (render_distortion_forward_kernel, front to back over the saved lists).  Backward: ONE compositing kernel
 * (render_distortion_backward_kernel: nine-float rows with the per-instance sum of dL/dm in column 0), a fold of column 0 per Gaussian into
 * dL/dz = -sum / z^2 (in the scratch, not in the binning buffer: a colour-only forward has no depth part there), and the per-Gaussian backward
 * das3r_raster_backward ends with, the antialiasing factor of an antialiased forward included.
 * Both calls read what ANY forward left in `saved`, as das3r_raster_aux_forward / _backward do: with or without out_invdepth, antialiased (hand
 * the flags back), every binning path and forward kernel — and, for the forward call, an evaluation forward.  args for the forward call:
 * P, image_width, image_height, debug; for the backward: args / in the forward was given.  The binning self-check is examined first.
 * out / totals are fully written.  grads: every buffer das3r_raster_backward would ask for, fully written; the colour gradient is written as
 * zeros.  grads->scratch: das3r_raster_distortion_backward_scratch_bytes(saved->capacity, P) bytes (the nine-float rows, then P floats),
 * 4-byte aligned, need not be initialised.  No floating-point atomics, no unordered adds: bit-identical from run to run; nothing needs
 * pre-zeroing.  P == 0 or nothing rendered: zeros.
 * DAS3R_ERR_INVALID_ARG with a das3r_last_error() message, before anything is launched: NULL structs, NULL out / dL_ddist / totals (backward),
 * NULL grads->scratch, grads->chain != NULL, and whatever das3r_raster_backward refuses.
 * One workgroup per tile in both kernels: few tiles with very long lists leave most of the chip idle.  The bucket-parallel form is owed — a
 * list segment combines associatively on (T, A, B, D) — see docs/ledger.md (cq). */
int das3r_raster_distortion_forward(const das3r_raster_args *args, const das3r_raster_saved *saved, float *out /* [H,W] */,
                                    float *totals /* [H,W] or NULL */, das3r_stream_t stream);
size_t das3r_raster_distortion_backward_scratch_bytes(int64_t capacity, int32_t P);
int das3r_raster_distortion_backward(const das3r_raster_args *args, const das3r_raster_in *in, const das3r_raster_saved *saved,
                                     const float *dL_ddist /* [H,W] */, const float *totals /* [H,W]: the forward call's */,
                                     const das3r_raster_grads *grads, das3r_stream_t stream);

/* ---- median depth and surface hits over a forward's lists, with adjoint (opt-in) ------------------------------------------------------
 * Additive symbols under ABI 16.  The depth of the Gaussian at which a ray's transmittance crosses a threshold — the surface depth of point
 * and mesh export, of depth evaluation, of the 2DGS / RaDe-GS depth and normal terms and of picking — and, as its by-product, which Gaussian
 * that is.  Like the distortion it is no blend of per-Gaussian channels: das3r_raster_aux_forward cannot produce it.
 * Definition.  Take the forward that left `saved`, a pixel whose colour was blended from list entries k = 0 .. n-1, and a threshold tau.
 *   - The entries are the colour's own.  The order, alpha (pair_alpha) and the stop at n_contrib[pixel] are the same.
 *   - T_k is the transmittance in front of entry k: T_0 = 1, T_{k+1} = T_k (1 - alpha_k).
 *   - hit = max { k < n : T_k > tau }.  This is the first entry behind which T <= tau, or the last contributor when the ray never gets that
 *     opaque.
 *   - T_0 = 1 > tau, so every pixel with a contributor has a hit.
 * Outputs, each a plane in caller memory and each fully written:
 *     depth         f32 [H,W]               z_hit, the fp32 view-space depth the forward saved in the splat record (rgbd.w)
 *                                           empty pixel: 0.0 exactly
 *     hit_gaussian  i32 [H,W], may be NULL  Gaussian index at the hit                                             empty pixel: -1
 *     hit_position  u32 [H,W], may be NULL  0-based position of the hit in its tile's list; the adjoint takes this back
 *                                           empty pixel: 0xFFFFFFFF
 * An empty pixel is one with n_contrib == 0.
 *   - Threshold.  0 < tau < 1.  0.5 is the median.  A smaller tau gives a deeper quantile.
 *   - No background term, no antialiasing special case.  The antialiasing factor is part of the saved opacity.
 *   - Adjoint.  For an image g [H,W], dL_dz[i] = sum over the pixels whose hit_gaussian is i of g[pixel].  This is the whole derivative of
 *     <g, depth> with respect to the Gaussians' view-space depths.  Every discrete decision (lists, order, stop, which entry is the hit) is
 *     held fixed, as for the aux and distortion backwards.  With g = 1 it is the number of pixels a Gaussian is the surface of.
 *   - Determinism.  No floating-point atomics, no unordered adds.  Both calls are bit-identical from run to run.  Nothing needs pre-zeroing.
 * Launches.  Forward: ONE kernel (render_median_forward_kernel, front to back over the saved lists; a wave leaves the walk once all its
 * pixels have T <= tau or are past their last contributor, the workgroup once its four waves have).  Adjoint: ONE compositing kernel
 * (render_median_adjoint_kernel: one float per list entry into the scratch — the sum of g, in a fixed pixel order, over the pixels whose hit
 * the entry is; 0 for every other entry), then the gather of das3r_raster_aux_adjoint at C = 1 into dL_dz [P] (=, or += with accumulate != 0;
 * fully written, zeros for a Gaussian that is nobody's hit, unless accumulate).  A hit_position at or past its tile's list length (the
 * empty marker, or garbage) contributes nothing and indexes nothing.
 * Both calls read what ANY forward left in `saved`, as das3r_raster_distortion_forward / das3r_raster_aux_adjoint do: with or without
 * das3r_raster_in.pre, with or without out_invdepth, antialiased, an evaluation forward, every binning path and forward kernel.  args supplies
 * P, image_width, image_height and debug.  The binning self-check is examined first.  scratch: das3r_raster_median_scratch_bytes(
 * saved->capacity) bytes (one float per list entry), 4-byte aligned, need not be initialised.  P == 0 or nothing rendered: the empty values,
 * and zeros to dL_dz unless accumulate.
 * DAS3R_ERR_INVALID_ARG with a das3r_last_error() message, before anything is launched: NULL structs, NULL depth, NULL dL_ddepth, NULL
 * hit_position (adjoint), NULL dL_dz, NULL scratch, and a threshold that is not inside (0, 1), NaN included.
 * One workgroup per tile in both kernels, as for the siblings; a long-list form is not part of these entries. */
int das3r_raster_median_forward(const das3r_raster_args *args, const das3r_raster_saved *saved, float threshold, float *depth /* [H,W] */,
                                int32_t *hit_gaussian /* [H,W] or NULL */, uint32_t *hit_position /* [H,W] or NULL */, das3r_stream_t stream);
size_t das3r_raster_median_scratch_bytes(int64_t capacity);
int das3r_raster_median_adjoint(const das3r_raster_args *args, const das3r_raster_saved *saved, const float *dL_ddepth /* [H,W] */,
                                const uint32_t *hit_position /* [H,W]: the forward call's */, float *dL_dz /* [P] */, int32_t accumulate,
                                float *scratch, das3r_stream_t stream);

/* ---- the normal-consistency regulariser: per-Gaussian normals, the normal of a depth image, the loss image (csrc/normals.hip) ----
 * Additive symbols under ABI 16.  The normal term of the surface-oriented splatting methods (2DGS, GOF, PGSR, RaDe-GS): the normal blended
 * from the Gaussians must agree with the normal of the rendered depth surface.  The blend itself is das3r_raster_aux_forward over a forward's
 * lists (three channels) and the depth is das3r_raster_median_forward's or alpha / inverse depth; what is declared here are the two ends.
 *
 * 1. PER-GAUSSIAN NORMALS.  Definition, for Gaussian i:
 *   - k = argmin_j scales[i][j].  Ties take the lowest j.
 *   - a = column k of R(q / |q|), q = rotations[i] = (r, x, y, z), R the matrix of quat_to_R in oracle/raster_oracle.c:
 *       R = [ 1 - 2 (y y + z z)   2 (x y - r z)       2 (x z + r y)     ]
 *           [ 2 (x y + r z)       1 - 2 (x x + z z)   2 (y z - r x)     ]
 *           [ 2 (x z - r y)       2 (y z + r x)       1 - 2 (x x + y y) ]
 *   - d = means3D[i] - campos.
 *   - flip = (a . d > 0).  A dot product of exactly 0 keeps a.
 *   - n_world = flip ? -a : a.
 *   - normals[i] = n_world taken into view space by the rotation part of args->viewmatrix, in the row-vector convention of the preprocess
 *     kernel: normals[i][j] = sum_c n_world[c] viewmatrix[4 c + j].
 *   - choice[i] = k | (flip << 2).
 * args supplies P, viewmatrix and campos only (and debug).
 * CAVEAT.  The rasterizer uses a raw quaternion as given.  For |q| != 1 the normal is the axis of the NORMALISED quaternion, not an
 * eigenvector of the sheared covariance the rasterizer builds from the raw one.  A quaternion whose squared norm is 0 or not finite has no
 * axis: its normal and its gradient are exact zeros.
 * The unit is compiled without FMA contraction: k and flip are plain IEEE fp32 decisions (the products and the two additions of a . d in
 * the order x, y, z).
 * Backward.  k and flip are read from choice: they are the forward's discrete decisions, held fixed.  The gradient goes to the raw
 * quaternion, through the normalisation: with g^ = dL/d(q / |q|), dL_drotations[i] = (g^ - q^ (q^ . g^)) / |q|.  Scales and means receive
 * none.  dL_drotations is fully written unless accumulate != 0 (then added to).
 * Launches: ONE kernel each, one thread per Gaussian, no LDS, no atomics; bit-identical from run to run.
 * DAS3R_ERR_INVALID_ARG with a das3r_last_error() message, before anything is launched: NULL args, P < 0, NULL viewmatrix / campos, and
 * any NULL array (a cov3D_precomp caller has no axes and cannot call this).  P == 0 returns DAS3R_OK and launches nothing.
 *
 * 2. DEPTH NORMALS AND THE LOSS IMAGE.  depth [H,W] is a view-space z image.  Per pixel (x, y):
 *   - The ray is r = (((2x+1)/W - 1) tanfovx, ((2y+1)/H - 1) tanfovy, 1): the rasterizer's pixel-centre convention.  The point is p = z r.
 *   - Tangents by central differences, in the form that does not cancel, with z+- = z(x+-1, y), r the centre pixel's ray and
 *     t_x = 2 tanfovx / W, t_y = 2 tanfovy / H the ray's step from one pixel to the next:
 *       dx = ((z+ - z-) r_x + (z+ + z-) t_x,  (z+ - z-) r_y,  z+ - z-)            = p(x+1, y) - p(x-1, y) = z+ (r + t_x e_x) - z- (r - t_x e_x)
 *       dy = ((z+ - z-) r_x,  (z+ - z-) r_y + (z+ + z-) t_y,  z+ - z-)  in y      = p(x, y+1) - p(x, y-1)
 *   - N_d = (dy x dx) / |dy x dx|.  This orientation faces the camera: a fronto-parallel plane gives (0, 0, -1), as the per-Gaussian
 *     normals of part 1 do.
 *   - loss = m (alpha - normal . N_d), m = mask if given, else 1.  With normal = sum_k w_k n_k and alpha = sum_k w_k this is
 *     sum_k w_k (1 - n_k . N_d) over the blended entries: 2DGS's term.
 *   - A pixel is VALID iff 1 <= x <= W-2 and 1 <= y <= H-2; its own z and its four neighbours' z are finite and > 0; |dy x dx|^2 is
 *     finite and > 0.  An invalid pixel gives exactly 0 for loss and depth_normal, and sends exactly 0 to every gradient, whatever NaN or
 *     garbage sits in depth there.  Images with no interior pixel (H < 3 or W < 3) produce all zeros.
 * Backward, for an upstream image g = dL_dloss: dL_dalpha = g m;  dL_dnormal = -g m N_d;  dL_ddepth in GATHER form — pixel q sums the
 * contributions of the four neighbours whose stencil reads z_q (left, right, upper, lower, in this order), each neighbour's cross product
 * recomputed.  A pixel's own z does not enter its own normal: it enters only its validity.  mask is a constant.
 * Launches: ONE kernel each; a workgroup takes a 32 x 8 tile of pixels and stages the depths of the tile and its halo (1 pixel forward, 2
 * backward: the radius-2 diamond) in LDS, every halo index clamped into the image before the load.  No floating-point atomics; nothing
 * needs pre-zeroing; every output is fully written; bit-identical from run to run.
 * DAS3R_ERR_INVALID_ARG with a das3r_last_error() message, before anything is launched: H, W <= 0, H * W > 2^30, a non-finite tanfov, and
 * any NULL pointer but mask and depth_normal. */
int das3r_gaussian_normals_forward(const das3r_raster_args *args, const float *rotations /* [P,4] */, const float *scales /* [P,3] */,
                                   const float *means3D /* [P,3] */, float *normals /* [P,3] */, uint8_t *choice /* [P] */, das3r_stream_t stream);
int das3r_gaussian_normals_backward(const das3r_raster_args *args, const float *rotations, const uint8_t *choice,
                                    const float *dL_dnormals /* [P,3] */, float *dL_drotations /* [P,4] */, int32_t accumulate, das3r_stream_t stream);
int das3r_normal_consistency_forward(int32_t H, int32_t W, float tanfovx, float tanfovy, const float *depth /* [H,W] view-space z */,
                                     const float *normal /* [3,H,W] */, const float *alpha /* [H,W] */, const float *mask /* [H,W] or NULL */,
                                     float *loss /* [H,W] */, float *depth_normal /* [3,H,W] or NULL */, das3r_stream_t stream);
int das3r_normal_consistency_backward(int32_t H, int32_t W, float tanfovx, float tanfovy, const float *depth, const float *normal,
                                      const float *mask, const float *dL_dloss /* [H,W] */, float *dL_ddepth /* [H,W] */,
                                      float *dL_dnormal /* [3,H,W] */, float *dL_dalpha /* [H,W] */, das3r_stream_t stream);

/* ---- introspection (used by the parity tests and the roofline accounting) ---- */

/* Byte offsets of the saved intermediates inside geom / binning / img for given extents. */
typedef struct {
    size_t geom_bytes, binning_bytes, img_bytes;
    /* geom */
    size_t depth_key;      /* u32[P]  fp32 depth bits, 0xFFFFFFFF = culled */
    /* xy / conic_opacity / rgbd are the three float4 fields of ONE 64-byte record per Gaussian (a tile's gather of a splat
     * touches one cache line instead of three): element g of each lives at its offset + g * splat_stride bytes */
    size_t xy;             /* f32[4] per record: pixel centre x, y + culling half extents hx, hy */
    size_t conic_opacity;  /* f32[4] per record */
    size_t rgbd;           /* f32[4] per record (r,g,b,depth) */
    size_t splat_stride;   /* bytes between consecutive Gaussians' records (64) */
    size_t clamped;        /* u8[P]    bit c set = channel c clamped */
    size_t tiles_touched;  /* u32[P] */
    size_t sorted_idx;     /* u32[P]   depth rank -> gaussian index */
    size_t offsets;        /* u32[P]   exclusive instance offset per depth rank */
    /* binning */
    size_t point_list;     /* u32[I]   gaussian index per instance, ordered (tile, depth, index) */
    /* img */
    size_t final_T;        /* f32[H*W] */
    size_t n_contrib;      /* u32[H*W] */
    size_t ranges;         /* u32[tiles,2] */
} das3r_raster_layout;

int das3r_raster_get_layout(int32_t P, int64_t capacity, int32_t W, int32_t H, das3r_raster_layout *out);

/* Optional per-kernel timing: when enabled, every kernel launch of the library is bracketed by HIP events recorded on
 * the launch stream.  das3r_profile_report synchronises and writes one line per kernel, "<kernel> <launches> <total_ms>\n",
 * into buf, then clears the records; returns bytes written or a negative status.  Single-threaded use (bench.py). */
void das3r_profile_enable(int on);
int das3r_profile_report(char *buf, size_t cap);

/* Test aid: one workgroup per CU (and a few more) fills the CU's whole LDS with `pattern` (e.g. 0x7FC00000 = NaN, 0xFFFFFFFF), so that
 * a following kernel that reads LDS it has not written sees it (tests/test_gpu_raster.py). */
int das3r_debug_poison_lds(uint32_t pattern, das3r_stream_t stream);

/* Test aid: OR `bits` into the binning self-check word of every forward from now on (0 switches it off again) — how the tests
 * prove that a failed binning is reported before the backward pass launches anything.  A call, not an environment variable:
 * nothing in the environment can make the shipped library report or compute anything else than it should. */
void das3r_debug_inject_fault(uint32_t bits);

/* Test aid (mutation test of the parity suite): what = 1 makes the block-walk compositing backward
 * (render_bwd_blk.hip, the kernel of the 1 M-splat headline and of the DAS3R training shape) evaluate exp(power) (1 + 1e-4) — the
 * kind of bias a "fast exp" or a packed-record shortcut would bring in; 0 switches it off.  tests/test_gpu_fullsize.py asserts that
 * the full-size oracle comparison FAILS under it.  A call, not an environment variable (see das3r_debug_inject_fault). */
void das3r_debug_mutate(uint32_t what);

/* Pair counters of the compositing kernels (bench.py: pairs per second).  enable != 0: zero the counters and count from now on;
 * enable == 0: stop, and read into out (may be NULL): out[0] (pixel, splat) pairs the forward compositing kernel evaluated, [1] the
 * same for the backward kernel, [2] / [3] their wave iterations (64 pairs each).  Costs one atomic per wave while enabled, nothing
 * otherwise.  Single-threaded use; synchronises the device. */
int das3r_pair_counters(int enable, uint64_t out[4]);

/* ABI 12.  Measurement aid (bench.py): the LIVE (pixel, splat) pairs of the forward that produced `saved` — list position below the pixel's
 * last contributor, power <= 0, alpha >= 1/255 (what upstream:forward.cu renderCUDA blends) — into out[0], and the (pixel, list
 * position) pairs below the pixels' last contributors into out[1].  A plain walk over the saved buffers; synchronises the stream. */
int das3r_raster_count_live_pairs(const das3r_raster_args *args, const das3r_raster_saved *saved, uint64_t out[2], das3r_stream_t stream);

/* The library reads its diagnostic / experiment switches (environment variables DAS3R_*) once, at the first
 * call; a process that changes them afterwards (tests, A-B tools) calls this to have them read again. */
void das3r_reload_switches(void);

/* Process-wide counters since load: out[0] forwards, [1] binning self-check words examined by the host, [2] of those with the
 * "a stalled look-back poll was rescued by the atomic read path" note (granule.h; informational), [3] failed self-checks. */
void das3r_get_stats(uint64_t out[4]);

/* ABI 13.  Forget what the calling thread has learnt about shapes on the current device (das3r_raster.h "State between calls": the
 * instance counts a speculative capacity is laid out from, the binning path, and — round 6 — which forward compositing kernel a shape
 * gets: one workgroup per tile or four, chosen from the skew of the tile lists the shape's earlier forwards met).  Every learnt path
 * computes the same lists and the same gradients; the two forward kernels round a pixel's transmittance differently in the last bit, so
 * a job that must end bit-identical whatever ran on its thread before it calls this first (das3r_amd.farm.run_sequence_job does): its
 * forwards then see the library in the state a fresh thread finds it in.  Costs the first forwards of the next shape their short cuts. */
int das3r_raster_forget_shapes(void);

/* ABI 13.  The part of that state which shows in the last bit of a result, for checkpoints: set == 0 reads {forward kernel of the current shape
 * (0: one workgroup per tile, 1: four), forwards of the shape so far — the kernel is re-decided from the tile lists every 512th} into
 * state[0 .. 1]; set != 0 forgets the shapes (as above) and hands state[] to the next shape the calling thread meets: a job resumed from a
 * checkpoint continues with the kernel, and the re-decision schedule, the killed job had (das3r_amd.train save_checkpoint / farm resume). */
int das3r_raster_learning(int32_t set, uint32_t state[2]);

/* 1 when the library was built with the superseded experiment kernels (make EXPERIMENTS=1: DAS3R_RENDER_BWD=mfma | stream,
 * DAS3R_SORT=classic), 0 for the shipped build; the parity tests of those kernels skip themselves on 0. */
int das3r_has_experiments(void);

/* The split preprocess (geometry kernel on the caller's stream, SH colour kernel on the library's side stream).  Which form a forward takes
 * depends on its shape alone: has_sh (SH rows given), the active degree, P, the binning path the forward is on — 0 the global depth
 * sort, 1 index-order emission with binning kernels of its own (local order, segmented), 2 emission fused into the preprocess kernel —
 * and no_backward (das3r_raster_saved.flags bit 3 on the way in: an evaluation forward keeps the fused kernel).
 * forced: what DAS3R_SPLIT_COLOUR says (das3r_split_colour_switch: -1 = "0", never; 1 = "1", wherever the split form can run; 0 = unset).
 * Both forms store the same bits.  Host-only, no device needed. */
int das3r_split_colour_rule(int32_t has_sh, int32_t sh_degree, int32_t P, int32_t binning_path, int32_t no_backward, int32_t forced);
int das3r_split_colour_switch(void);

/* ---- the binning-path policy on a caller's own state (test aid) ------------------------------------------------------------------
 * Additive symbols under ABI 16 (no struct and no existing entry point changes).  What das3r_raster_forward learns about a shape and what
 * its next forward does with it — binning path, back-off to the global sort, speculative capacity, compositing kernels — is host
 * arithmetic (csrc/path_policy.h); these calls run exactly those functions on the state struct the caller passes, so that a test can
 * script any sequence of forwards (inputs, delivered count, mailbox words) and look at every plan and every resulting state.
 * Host-only: no device needed, no HIP call, and neither the calling thread's library state nor the DAS3R_* switches are looked at or
 * changed (what the policy reads of them is in das3r_path_policy_inputs).  Flags are 0 / 1. */
typedef struct {
    int32_t P, W, H;              /* the shape the state is about */
    int64_t last_I, peak_I;       /* the last forward's count (-1: none yet), the slowly forgotten largest one */
    int32_t radix_left, backoff;  /* forwards still to spend on the global sort, and what the next failure costs */
    uint32_t gen;                 /* generation: what the kernels' mailbox words name (never 0 once a shape was met) */
    int32_t seg_extra, last_seg, fine;
    uint32_t forwards, clean, longest;
    int32_t resume_valid, resume_fine;   /* das3r_raster_learning(set): waiting for the next shape */
    uint32_t resume_forwards;
} das3r_path_policy_state;
typedef struct {
    int32_t P, W, H, ntiles, tbits, tile_passes;   /* tbits: bits of a tile id; tile_passes = (tbits + 7) / 8 */
    uint32_t too_long, want_bits;                  /* the two mailbox words as read before the forward (0: not raised) */
    int32_t forced;                                /* DAS3R_BINNING: 0 unset, 1 local, -1 radix, 2 seg, 3 seg3, 4 bucket, 5 cells */
    int32_t onesweep;                              /* 1 except with DAS3R_SORT=classic of an experiments build */
    int64_t capacity_hint;                         /* das3r_raster_args.capacity_hint */
    int32_t capacity_exact;                        /* DAS3R_CAPACITY=exact */
} das3r_path_policy_inputs;
typedef struct {
    int32_t local, seg, seg_bits, seg_passes;      /* local order / segmented path (neither: global sort); bucket bits and passes of the latter;
                                                      seg == 2: segmented emission and passes, the lists finished by the compositing kernel */
    int32_t speculate, decide_fine;
    uint32_t gen;
    int32_t cells;                                 /* with seg == 2: the instances are partitioned by reserved ranges and finished per cell
                                                      (csrc/cell_sort.hip) instead of by the stable passes; in what used to be padding */
    int64_t cap;                                   /* with speculate */
} das3r_path_policy_plan;
void das3r_debug_path_policy_fresh(das3r_path_policy_state *state, uint32_t gen);   /* the state of a thread that has met no shape */
void das3r_debug_path_policy_plan(das3r_path_policy_state *state, const das3r_path_policy_inputs *in, das3r_path_policy_plan *plan);
/* the forward's count has arrived; 1: a forward that planned the local order at its exact size takes the global sort after all */
int das3r_debug_path_policy_count(das3r_path_policy_state *state, const das3r_path_policy_inputs *in, const das3r_path_policy_plan *plan, int64_t I);
/* a forward with plan.decide_fine has measured its tile lists; returns state->fine */
int das3r_debug_path_policy_skew(das3r_path_policy_state *state, uint32_t longest, uint32_t crowd16, int64_t cap, int32_t ntiles);
uint32_t das3r_debug_path_policy_hint(const das3r_path_policy_state *state);   /* das3r_raster_saved.flags bits 0 and 8 - 15 of a `fine` forward */
void das3r_debug_path_policy_forget(das3r_path_policy_state *state);           /* das3r_raster_forget_shapes */
void das3r_debug_path_policy_resume(das3r_path_policy_state *state, uint32_t fine, uint32_t forwards);   /* das3r_raster_learning(set) */
int das3r_debug_seg_dbits(int32_t tbits, int32_t passes);   /* depth-bucket bits `passes` partition passes leave beside tbits bits of tile id */

/* ---- the switches and the compositing-kernel choice on a caller's own values (test aid) -------------------------------------------
 * Additive symbols under ABI 16.  What every DAS3R_* spelling means and which compositing kernel a forward and a backward launch is host
 * arithmetic (csrc/kernel_choice.h); these calls run exactly those functions.  Host-only: no device needed, no HIP call; neither the process
 * environment nor the switches the library itself last read are looked at or changed.  Flags are 0 / 1.
 * Kernel kinds: forward 0 auto, 1 quad, 2 rows, 3 lanes, 4 slices, 5 fine (regions); backward 0 auto, 1 dpp, 2 mfma, 3 scan, 5 stream, 6 blk,
 * 7 fine (regions). */
typedef struct {
    int32_t sort_ipl, sort_classic, rect_upstream, verbose, binning, capacity_exact, fused_emit_off, no_sh_stage;
    int32_t render_fwd, render_bwd;                    /* the forced kernel kinds (0: none) */
    int32_t render_bwd_mb, render_bwd_atomic;          /* entries per round of a DAS3R_RENDER_BWD spelling (0: none given); scana... */
    int32_t render_bwd_pix, render_bwd_occ;            /* blk...p<N>, blk...o<N> */
    int32_t render_bwd_strips;                         /* fine...q: 1, fine...s: 2 */
    int32_t tile_chunk, scan_items, deterministic, tile_lpt_off, bwd_reduce_set, bwd_reduce_shfl, ablate_set, ablate, tickets;
    int32_t bwd_pad_lds, fwd_pad_lds, bwd_buckets, fwd_no_prefetch, split_colour, tile_strip;
} das3r_switches;
typedef struct {
    int32_t kernel, mb, slices;                        /* kind (never 0), entries per round, workgroups per tile of the bucket-parallel replay */
    int32_t pix, occ, strips, atomic_flush;            /* the forms of blk (pix, occ), of the region walk (strips) and of scan (atomic_flush) */
} das3r_bwd_choice;
typedef struct {
    int32_t kernel, quad_lanes, row_private, tile_lpt; /* kind (never 0); the predicates behind it; the tiles longest list first */
} das3r_fwd_choice;
/* parses the n (name, value) pairs as if they were the environment; experiments: also the variables only `make EXPERIMENTS=1` builds read */
void das3r_debug_parse_switches(const char *const *names, const char *const *values, int32_t n, int32_t experiments, das3r_switches *out);
/* fwd_flags: das3r_raster_saved.flags of the forward */
void das3r_debug_choose_backward(const das3r_switches *sw, int64_t num_rendered, int32_t ntiles, uint32_t fwd_flags, das3r_bwd_choice *out);
/* local_lists: the tile lists are in local depth order; prefer_regions: das3r_path_policy_state.fine */
void das3r_debug_choose_forward(const das3r_switches *sw, int32_t ntiles, int64_t capacity, int32_t local_lists, int32_t prefer_regions,
                                das3r_fwd_choice *out);
int das3r_debug_has_invdepth_form(int32_t backward, int32_t kernel);      /* can the (backward != 0: backward) kernel kind run with an inverse-depth map */
const char *das3r_debug_kernel_name(int32_t backward, int32_t kernel);    /* the kind's name in DAS3R_RENDER / DAS3R_RENDER_BWD and in error messages */

/* ---- the form of the per-Gaussian backward kernel on a caller's own values (test aid) -----------------------------------------------
 * Additive symbols under ABI 16.  Which of its instantiations preprocess_backward_kernel is launched as is host arithmetic
 * (csrc/preprocess_choice.h); these calls run exactly those functions.  Host-only: no device needed, no HIP call.  Flags are 0 / 1. */
typedef struct {
    int32_t has_sh, has_cov;                        /* SH rows / cov3D given */
    int32_t M, sh_degree;
    int32_t shs_aligned16, dL_dshs_aligned16;       /* 16-byte alignment of in->shs and of grads->dL_dshs */
    int32_t no_sh_stage;                            /* das3r_switches.no_sh_stage */
    int32_t jac_saved;                              /* das3r_raster_saved.flags bit 2: the forward left the colour's Jacobian planes */
    int32_t chained, quad_rows;                     /* grads->chain given; quadrant rows from the compositing backward (experiments build) */
    int32_t depth, aa;                              /* das3r_raster_backward_depth; das3r_raster_saved.flags bit 4 */
} das3r_preprocess_backward_inputs;
typedef struct {
    int32_t has_sh, has_cov, stage_in, stage_out, deg0, chain, depth, jac, aa;   /* the kernel's template arguments, in their order */
    int32_t base_index;                             /* out: position of the base form in the list of instantiated ones (-1: not instantiated) */
    int32_t sh_rows_staged;                         /* out: the forward's rule on the same inputs (its SH rows come in through LDS) */
} das3r_preprocess_form;
/* returns why a chained call is refused: 0 not refused (or not chained), 1 no SH rows, 2 cov3D given, 3 a staged SH layout, 4 quadrant rows */
int das3r_debug_choose_preprocess_backward(const das3r_preprocess_backward_inputs *in, das3r_preprocess_form *out);
/* the raw name das3r_profile_report lists a launch of the form under (reads the nine flags); null: not instantiated */
const char *das3r_debug_preprocess_backward_name(const das3r_preprocess_form *form);

/* ---- TSDF fusion of depth images into a voxel grid, and a mesh out of it (csrc/tsdf.hip) ---------------------------------------------
 * Additive symbols under ABI 16.  The last step of the 2DGS recipe: the per-view surface depths (das3r_raster_median_forward) are fused
 * into one truncated signed distance field, and a triangle mesh with normals and colours is taken from it by marching tetrahedra.
 *
 * The grid: dims = (nx, ny, nz), origin = the corner of voxel (0, 0, 0) in world units, edge `voxel`; voxel (i, j, k) has its centre at
 * origin + (i + 1/2, j + 1/2, k + 1/2) * voxel and the linear index (k * ny + j) * nx + i.  Dense fp32 tensors tsdf [nz, ny, nx],
 * weight [nz, ny, nx] and, optionally, colour [3, nz, ny, nx]; a fresh grid holds tsdf 1, weight 0, colour 0.  At most 2^28 voxels.
 *
 * das3r_tsdf_integrate: V views in one call.  viewmatrix: V x 16 floats in DEVICE memory, each in the layout das3r_raster_args.viewmatrix
 * has; tanfovx / tanfovy: V floats each in HOST memory (they are checked before anything is launched and travel as kernel arguments);
 * depth [V, H, W]: view-space z (what das3r_raster_median_forward writes), colour_img [V, 3, H, W] (required iff the grid has colour),
 * weight_img [V, H, W] or NULL (1 everywhere).  Per voxel, for each view in index order, in fp32 without fused multiply-adds, every sum
 * left to right:
 *   1. (xc, yc, zc) = centre * viewmatrix (row vector);  skip unless zc > near_z
 *   2. u = ((xc / zc) / tanfovx + 1) * (W / 2), v likewise (pixel x covers the rays ((2 x + 1) / W - 1) * tanfovx, as in
 *      das3r_normal_consistency_forward);  skip unless 0 <= u < W and 0 <= v < H;  px = floor(u), py = floor(v)
 *   3. d = depth[v, py, px]: skip unless d > 0 and finite;  w = weight_img[v, py, px] or 1: skip unless w > 0 and finite
 *   4. sdf = d - zc;  skip if sdf < -trunc (hidden behind the surface);  ts = min(1, sdf / trunc)
 *   5. Wn = Wt + w;  T = (T * Wt + ts * w) / Wn;  each colour channel the same way;  Wt = Wn
 * The call continues from what the grid holds: per view and per batch are the same arithmetic, bit for bit (more than
 * DAS3R_TSDF_MAX_VIEWS views are taken in chunks of that many launches).  das3r_amd/tsdf.py integrate_torch is this rule in torch ops.
 * One kernel per chunk, a thread per voxel; no atomics.  Refused with DAS3R_ERR_INVALID_ARG before any launch: NULL grid or depth, a
 * non-positive or non-finite voxel, trunc or tanfov, a dim < 1, more than 2^28 voxels, a colour image without a colour grid or the reverse.
 *
 * das3r_tsdf_extract_count / _emit: the mesh.  A voxel is VALID iff weight > 0 and tsdf is finite, INSIDE iff it is valid and tsdf < 0.
 * Vertices: voxel p owns the seven lattice edges p -> p + d, d = +x, +y, +z, +x+y, +x+z, +y+z, +x+y+z (types 0 - 6); an owned edge inside
 * the grid carries a vertex iff both ends are valid and exactly one is inside: with a = tsdf(p), b = tsdf(p + d), s = a / (a - b), at
 * origin + (p + 1/2 + s d) * voxel, with the lerp of the two colours and the normalised lerp of the two grid gradients (per axis the central
 * difference where both neighbours are valid, one-sided where one is, 0 where neither; it points to +tsdf, free space; (0, 0, 0) where
 * the length is zero or not finite).  Vertices are ordered by (owner's linear index, type).
 * Triangles: cube (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, is active iff its eight corners are valid, and splits into the six Kuhn
 * tetrahedra p0 -> p1 -> p2 -> p3 from its low to its high corner, the axes added in the orders xyz, xzy, yxz, yzx, zxy, zyx.  With I / O
 * the inside / outside corners of a tetrahedron in path order and XY the vertex on the edge between X and Y: 1 inside: (I0O0, I0O1, I0O2);
 * 3 inside: (O0I0, O0I1, O0I2); 2 inside: (I0O0, I0O1, I1O1), (I0O0, I1O1, I1O0); the last two indices swapped where a table of integer
 * determinants says so, so that every normal points from the inside corners to the outside ones.  Triangles are ordered by (cube's linear
 * index, tetrahedron, triangle); indices are int32 into the vertex list.
 * count: the per-voxel edge masks and triangle counts, their exclusive bases, and totals[0..1] = (Nv, Nf) in device memory — the one host
 * read between the two calls.  emit: vertices [Nv, 3], normals [Nv, 3], colours [Nv, 3] (iff the grid has colour), faces [Nf, 3]; with
 * Nv = Nf = 0 nothing is launched.  workspace: das3r_tsdf_extract_workspace_bytes(dims) bytes, 4-byte aligned, untouched between the two
 * calls; its first nvox uint32 words hold (edge mask | triangle count << 8) per voxel after count.  Separate launches, no atomics: two
 * runs are bit-identical. */
#define DAS3R_TSDF_MAX_VIEWS 16          /* views per launch of das3r_tsdf_integrate */
#define DAS3R_TSDF_MAX_VOXELS (1 << 28)
#define DAS3R_TSDF_GROUP_VOXELS 256
int das3r_tsdf_integrate(const int32_t *dims, const float *origin, float voxel, float *tsdf, float *weight, float *colour, int32_t V,
                         const float *viewmatrix, const float *tanfovx, const float *tanfovy, int32_t H, int32_t W, const float *depth,
                         const float *colour_img, const float *weight_img, float trunc, float near_z, das3r_stream_t stream);
size_t das3r_tsdf_extract_workspace_bytes(const int32_t *dims);   /* 0: the dims are refused */
int das3r_tsdf_extract_count(const int32_t *dims, const float *tsdf, const float *weight, char *workspace, int32_t *totals, das3r_stream_t stream);
int das3r_tsdf_extract_emit(const int32_t *dims, const float *origin, float voxel, const float *tsdf, const float *weight, const float *colour,
                            const char *workspace, int32_t Nv, int32_t Nf, float *vertices, float *normals, float *colours, int32_t *faces,
                            das3r_stream_t stream);
/* Test aids, host-only (no device needed, no HIP call): the kernels' own per-voxel functions over HOST memory (viewmatrix included), and the
 * winding table (word t: bit 2 c + k set where triangle k of case c of tetrahedron t has its last two indices swapped; case bit q = path
 * corner q inside).  _extract_host: called with vertices == NULL it counts into totals[0..1], called again with the arrays it emits. */
int das3r_debug_tsdf_integrate_host(const int32_t *dims, const float *origin, float voxel, float *tsdf, float *weight, float *colour, int32_t V,
                                    const float *viewmatrix, const float *tanfovx, const float *tanfovy, int32_t H, int32_t W, const float *depth,
                                    const float *colour_img, const float *weight_img, float trunc, float near_z);
int das3r_debug_tsdf_extract_host(const int32_t *dims, const float *origin, float voxel, const float *tsdf, const float *weight, const float *colour,
                                  char *workspace, int32_t *totals, float *vertices, float *normals, float *colours, int32_t *faces);
void das3r_debug_tsdf_swap_table(uint32_t *out /*[6]*/);

/* ---- Mesh clean-up: connected components, small pieces dropped (csrc/mesh.hip) --------------------------------------------------------
 * Additive symbols under ABI 16.  Imperfectly masked movers and faint floaters leave small closed blobs in a fused TSDF, and the extraction
 * turns each into a piece of mesh.  These calls label the connected pieces of a mesh, select the large ones and remap the faces; vertex
 * attributes are moved by das3r_prune_compact with the vertex_dst of the selection.  Everything is integer-valued: two runs are
 * bit-identical, and das3r_amd/mesh.py components_torch is the same definition in torch ops.
 *
 * Mesh and graph.  A mesh is Nv vertices and faces [Nf, 3] int32.  A face is GOOD iff its three indices lie in [0, Nv).  A good face joins
 * its three vertices (a face with a repeated index joins the distinct ones); a bad face joins nothing.  Connectivity is by shared VERTEX,
 * not by shared edge: union-find over vertices needs no edge map, and on the extraction's meshes the two notions agree.
 *
 * das3r_mesh_components.  vertex_label[v] = the smallest vertex index in v's component (canonical: independent of any order of execution);
 * face_label[f] = vertex_label[faces[f][0]] for a good face, -1 for a bad one; face_count[r] = the good faces of the component of root r
 * (vertex_label[r] == r), 0 at every non-root ([Nv] words); info[4]: [0] components, singletons included, [1] components with at least one
 * face, [2] bad faces, [3] a give-up word, 0 on success.  Four launches: init; a thread per face that unions (a, b) and (b, c) in a
 * union-find with minimum roots (parent[v] <= v always; the larger root is hooked under the smaller with an agent-scope atomic minimum; a
 * find walks strictly decreasing indices, a union iteration that does not hook goes on with a strictly smaller pair; no thread waits for
 * another; inside the launch the parent array is touched only with agent-scope atomic loads and minima, path halving included); a thread
 * per vertex that flattens; a wave per 1024 faces for face_label and the counts (one integer atomic per run of equal labels).  Every loop
 * also carries an iteration cap that sets info[3].  The call copies info to info_host (HOST memory, [4]) and waits for the stream: its one
 * host read; a non-zero info[3] is DAS3R_ERR_OVERFLOW.  Nv == 0 or Nf == 0 launch only what they need (Nf == 0: Nv singletons).
 * workspace: das3r_mesh_components_workspace_bytes(Nv, Nf) bytes (0: the sizes are refused), 4-byte aligned; das3r_mesh_filter_select
 * may be given the same one.
 *
 * Keep rule (host arithmetic: das3r_amd/mesh.py keep_threshold).  Parameters min_faces >= 0 and keep_largest = K >= 0.  With c_1 >= c_2 >= ...
 * the face counts of the face-bearing components, t = max(1, min_faces, c_K), the c_K term only when 1 <= K <= their number.  A component
 * is kept iff face_count >= t: ties at c_K are all kept, so no tie-break is needed; faceless vertices always go.
 *
 * das3r_mesh_filter_select takes the threshold t = min_count >= 1.  A vertex is kept iff its component is kept, a face iff it is good and
 * its component is kept; both keep their relative order (stable).  vertex_dst [Nv] / face_dst [Nf]: the new row, -1 = dropped; totals[2] =
 * (kept vertices, kept faces) in device memory, copied to totals_host (HOST, [2]): its one host read.  Flags plus per-group counts, a
 * one-workgroup scan, then ranks (das3r_prune_select's pattern and its scan and rank kernels).
 * das3r_mesh_filter_faces: out_faces[face_dst[f]] = vertex_dst[faces[f]] for every kept face; kept_faces == 0 launches nothing.
 *
 * Refused with DAS3R_ERR_INVALID_ARG and a das3r_last_error() message before any launch: a negative size or one above 2^30, a NULL array
 * that the sizes make necessary, a misaligned workspace, min_count < 1, kept counts outside [0, Nv] / [0, Nf]. */
size_t das3r_mesh_components_workspace_bytes(int32_t Nv, int32_t Nf);
int das3r_mesh_components(int32_t Nv, int32_t Nf, const int32_t *faces, int32_t *vertex_label, int32_t *face_label, int32_t *face_count,
                          int32_t *info /* device [4] */, int32_t *info_host /* host [4] */, char *workspace, das3r_stream_t stream);
int das3r_mesh_filter_select(int32_t Nv, int32_t Nf, const int32_t *vertex_label, const int32_t *face_label, const int32_t *face_count,
                             int32_t min_count, int32_t *vertex_dst, int32_t *face_dst, int32_t *totals /* device [2] */,
                             int32_t *totals_host /* host [2] */, char *workspace, das3r_stream_t stream);
int das3r_mesh_filter_faces(int32_t Nv, int32_t Nf, int32_t kept_vertices, int32_t kept_faces, const int32_t *faces, const int32_t *face_dst,
                            const int32_t *vertex_dst, int32_t *out_faces /* [kept_faces, 3] */, das3r_stream_t stream);
/* Test aid, host-only (no device needed, no HIP call): the kernels' own union and find run serially over HOST memory. */
int das3r_debug_mesh_components_host(int32_t Nv, int32_t Nf, const int32_t *faces, int32_t *vertex_label, int32_t *face_label, int32_t *face_count,
                                     int32_t *info /* [4] */);

int das3r_abi_version(void);
const char *das3r_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DAS3R_RASTER_H */
