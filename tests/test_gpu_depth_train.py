"""GPU tests of depth-supervised training (INTEGRATION.md "Depth supervision"): the fused inverse-depth L1 kernel against the formula, one
step against a float64 restatement (a DenseTrainer subclass that renders 1/z with the dense oracle and adds the term), the three forms of
the fused iteration against each other, the switched-off step against the step of a camera that carries no depth target, the schedule end
to end, and resume."""
import copy
import ctypes as C
import math
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.dense_oracle import rasterize_dense
from oracle.dense_trainer import DenseTrainer

pytestmark = pytest.mark.gpu

PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
NAMES = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation", "conf_static": "_conf_static", "Q": "Q", "T": "T"}
DEPTH_KERNELS = ("depth_l1_kernel", "depth_l1_finish_kernel", "depth_pass_inputs_kernel", "depth_fold_kernel")


def _is_depth_forward(raw_name):
    """Raw profiler names are the launch sites' text: the DEPTH instantiation is the last template flag of every forward compositing kernel
    (render_forward_rows_kernel<PREFETCH> has one flag without it, two with)."""
    if not raw_name.startswith("render_forward"):
        return False
    if raw_name.startswith("render_forward_rows_kernel"):
        return raw_name.replace(" ", "").endswith(",true>")
    return raw_name.replace(" ", "").endswith("<true>")


def _depth_launches(raw_report):
    """{what: launches} of everything a depth step adds to a photometric one."""
    out = {k: 0 for k in DEPTH_KERNELS + ("depth_forward", "colour_forward")}
    for name, (n, _ms) in raw_report.items():
        base = name.split("<")[0]
        if base in DEPTH_KERNELS:
            out[base] += n
        elif name.startswith("render_forward"):
            out["depth_forward" if _is_depth_forward(name) else "colour_forward"] += n
    return out


# ---------------------------------------------------------------------------------------------------------------- 5. kernel vs formula
def _random_maps(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    D = 0.05 + torch.rand(H, W, generator=g)
    T = 0.05 + torch.rand(H, W, generator=g)
    T[torch.rand(H, W, generator=g) < 0.01] = 0.0
    m = (torch.rand(H, W, generator=g) > 0.25).float()
    s = torch.rand(H, W, generator=g)
    s[torch.rand(H, W, generator=g) < 0.2] = 0.0
    D[0, :3] = T[0, :3]   # exact ties: |x| at 0 has gradient 0
    return D, T, m, s


def _run_kernel(D, T, m, s, weight, grad_loss, out8_before):
    from das3r_amd import _lib
    lib = _lib.load()
    H, W = D.shape
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    d = torch.full((H, W), float("nan"), device="cuda")
    partials = torch.full((int(lib.das3r_depth_l1_blocks(H, W)), 8), float("nan"), device="cuda")   # (scratch: need not be zeroed)
    out8 = out8_before.clone()
    g = None if grad_loss is None else torch.tensor([grad_loss], device="cuda")
    rc = lib.das3r_depth_l1(H, W, p(D), p(T), p(m), p(s), C.c_float(weight), p(g), p(d), p(partials), p(out8), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "das3r_depth_l1")
    torch.cuda.synchronize()
    return d, out8


@pytest.mark.parametrize("with_static,grad_loss", [(False, None), (True, None), (True, 2.5)])
@pytest.mark.parametrize("H,W", [(208, 512), (80, 128), (37, 53)])
def test_depth_l1_kernel_against_the_formula(H, W, with_static, grad_loss):
    """das3r_depth_l1 on random maps against das3r_amd.losses.depth_l1 in float64.  Value: relative error <= 1e-5 (a fixed-order fp32 sum of
    <= 1.1e5 non-negative terms); gradient: rtol 1e-6 against the fp32 closed form (three multiplies and one divide at 6e-8 each); exact zeros
    where m * s == 0 (NaN targets there included); two runs bit-identical; out8[0] grows by exactly out8[6]."""
    from das3r_amd.losses import depth_l1
    assert (W % 4 != 0) == (W == 53)
    D, T, m, s = _random_maps(H, W, 17 + H)
    if not with_static:
        s = None
    ms = m if s is None else m * s
    off = ms == 0
    assert bool(off.any()) and not bool(off.all())
    T_nan = T.clone()
    T_nan[off] = float("nan")
    weight = 0.37
    ref = float(depth_l1(D.double(), T.double(), m.double(), None if s is None else s.double()))
    cu = lambda t: None if t is None else t.cuda().contiguous()
    before = torch.tensor([0.5, 1.0, 2.0, 3.0, 4.0, 9.0, 9.0, 7.0], device="cuda")
    d1, o1 = _run_kernel(cu(D), cu(T_nan), cu(m), cu(s), weight, grad_loss, before)
    d2, o2 = _run_kernel(cu(D), cu(T_nan), cu(m), cu(s), weight, grad_loss, before)
    assert torch.equal(d1, d2) and torch.equal(o1, o2), "two runs must be bit-identical"
    o = o1.cpu()
    print(f"[depth_l1 {H}x{W} static={with_static} grad_loss={grad_loss}] value {float(o[5]):.9g} vs float64 {ref:.9g}: rel {abs(float(o[5]) - ref) / ref:.3g}")
    assert abs(float(o[5]) - ref) <= 1e-5 * ref, (float(o[5]), ref)
    assert abs(float(o[6]) - weight * float(o[5])) <= 1e-6 * abs(float(o[6]))
    assert float(o[0]) == float(before[0].cpu() + o[6]), "out8[0] after the call = its value before + out8[6] (one fp32 add)"
    assert torch.equal(o[1:5], before[1:5].cpu()) and float(o[7]) == 7.0
    # gradient: the fp32 closed form grad_loss * w * m s sgn((D - D*) m s) / (H W)
    gl = 1.0 if grad_loss is None else grad_loss
    e = (D - T) * ms
    closed = (torch.tensor(gl * weight, dtype=torch.float32) * ms * torch.sign(e)) / float(H * W)
    got = d1.cpu()
    assert torch.isfinite(got).all()
    assert bool((got[off] == 0).all()), "exact zeros where m * s == 0"
    assert bool((got[0, :3] == 0).all()), "d|x|/dx at 0 is 0"
    rel = ((got - closed).abs() / closed.abs().clamp_min(1e-30))[closed != 0]
    print(f"   gradient: max relative error {float(rel.max()):.3g} over {int(rel.numel())} live pixels")
    assert torch.allclose(got, closed, rtol=1e-6, atol=0.0)


def test_fused_depth_l1_loss_is_an_autograd_function_of_invdepth_alone():
    from das3r_amd.fused import depth_l1_loss
    from das3r_amd.losses import depth_l1
    D, T, m, s = (t.cuda() for t in _random_maps(40, 64, 5))
    D1 = D[None].clone().requires_grad_(True)   # [1, H, W], as the rasterizer returns it
    s1 = s.clone().requires_grad_(True)
    assert float(depth_l1_loss(D, T, m, s, weight=0.25)) == 0.25 * float(depth_l1_loss(D, T, m, s))   # (a power of two: exact)
    (3.0 * depth_l1_loss(D1, T, m, s1)).backward()
    D2 = D[None].clone().requires_grad_(True)
    (3.0 * depth_l1(D2, T, m, s)).backward()
    assert s1.grad is None
    assert D1.grad.shape == D2.grad.shape and torch.allclose(D1.grad, D2.grad, rtol=1e-6, atol=0.0)
    assert abs(float(depth_l1_loss(D, T, m, None)) - float(depth_l1(D.double(), T.double(), m.double()))) <= 1e-5 * float(depth_l1(D.double(), T.double(), m.double()))


# ------------------------------------------------------------------------------------------- the float64 restatement of a depth step
class DepthTrainer(DenseTrainer):
    """DenseTrainer with the inverse-depth L1 term: `render` also renders D = sum_i (1/z_i) alpha_i T_i (a second rasterize_dense call with
    colors_precomp = 1/z and no background; autograd carries 1/z back to the means), `loss_of` adds w * mean |(D - D*) m s| with
    s = conf_static[uid] as a constant.  targets: {uid: (D* [H, W], m [H, W])}."""

    def __init__(self, *a, targets=None, depth_weight=0.0, **k):
        super().__init__(*a, **k)
        self.targets, self.depth_weight, self.invdepth = targets or {}, depth_weight, None

    def render(self, uid, bg, pose=None):
        p, cam = self.p, self.cams[uid]
        pose = torch.cat([p["Q"][uid], p["T"][uid]]) if pose is None else pose
        q = pose[:4] / pose[:4].norm()
        w, x, y, z = q
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]).reshape(3, 3)
        means3D = p["xyz"] @ R.t() + pose[4:]
        a, b = pose[:4], p["rotation"]
        rot = torch.stack([a[0] * b[:, 0] - a[1] * b[:, 1] - a[2] * b[:, 2] - a[3] * b[:, 3],
                           a[0] * b[:, 1] + a[1] * b[:, 0] + a[2] * b[:, 3] - a[3] * b[:, 2],
                           a[0] * b[:, 2] - a[1] * b[:, 3] + a[2] * b[:, 0] + a[3] * b[:, 1],
                           a[0] * b[:, 3] + a[1] * b[:, 2] - a[2] * b[:, 1] + a[3] * b[:, 0]], 1)
        opac = torch.sigmoid(p["opacity"]) * p["conf_static"].reshape(-1, 1)[self.mask]
        dev = p["xyz"].device
        H, W = cam["gt"].shape[1:]
        common = dict(scales=torch.exp(p["scaling"]), rotations=rot, image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5),
                      tanfovy=math.tan(cam["fovy"] * 0.5), scale_modifier=1.0, viewmatrix=torch.eye(4, dtype=self.dtype, device=dev),
                      projmatrix=cam["proj_T"].to(self.dtype), sh_degree=self.active_deg, campos=torch.zeros(3, dtype=self.dtype, device=dev),
                      dtype=self.dtype)
        means2D = torch.zeros(p["xyz"].shape[0], 3, dtype=self.dtype, device=dev, requires_grad=True)
        color, _, _ = rasterize_dense(means3D, means2D, opac, shs=torch.cat([p["f_dc"], p["f_rest"]], 1), bg=bg, **common)
        inv = (1.0 / means3D[:, 2].clamp_min(1e-6))[:, None].expand(-1, 3)   # (the view matrix is the identity: z is the third coordinate)
        depth, _, _ = rasterize_dense(means3D, means2D, opac, colors_precomp=inv, bg=torch.zeros(3, dtype=self.dtype, device=dev), **common)
        self.invdepth = depth[0]
        return color, means2D

    def loss_of(self, uid, bg):
        loss, psnr_frame, means2D = super().loss_of(uid, bg)
        if self.depth_weight > 0 and uid in self.targets:
            T, m = (t.to(self.dtype) for t in self.targets[uid])
            s = self.p["conf_static"][uid].detach()
            self.depth_pure = ((self.invdepth - T) * m * s).abs().mean()
            loss = loss + self.depth_weight * self.depth_pure
        return loss, psnr_frame, means2D


def _pair(frames, W, H, seed, iterations, fused=False, generic=True, weights=(1.0, 1.0), carry=True, dtype=torch.float64):
    """tests/test_gpu_trainstep.py's `_pair` (same scene recipe) with depth targets on the cameras, the term's weights in OptimParams and the
    DepthTrainer restatement.  carry=False: cameras without the two attributes."""
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    seq = synthetic_sequence(frames=frames, W=W, H=H, focal=0.9 * W, n_splats=1500, seed=seed)
    model, cams = build_from_sequence(copy.deepcopy(seq), depth_targets=carry)
    if generic:
        gen = torch.Generator().manual_seed(7 + seed)
        with torch.no_grad():
            model._scaling += 0.4 * torch.randn(model._scaling.shape, generator=gen).cuda()
            model._rotation.copy_(torch.nn.functional.normalize(torch.randn(model._rotation.shape, generator=gen)).cuda())
    opt = OptimParams(iterations=iterations, depth_l1_weight_init=weights[0], depth_l1_weight_final=weights[1])
    model.training_setup(opt, fused=fused)
    params = dict(xyz=model._xyz, f_dc=model._features_dc, f_rest=model._features_rest, opacity=model._opacity, scaling=model._scaling,
                  rotation=model._rotation, conf_static=model._conf_static, Q=model.Q, T=model.T, mask=model.aggregated_mask)
    cameras = [dict(gt=c.original_image, fovx=c.FoVx, fovy=c.FoVy, proj_T=c.projection_matrix) for c in cams]
    targets = {c.uid: (c.invdepthmap, c.depth_mask) for c in cams} if carry else {}
    dense = DepthTrainer(params, cameras, iterations=iterations, targets=targets, depth_weight=weights[0], dtype=dtype)
    return model, cams, opt, dense, seq


# ------------------------------------------------------------------------------------------- 6. one step against the restatement
@pytest.mark.parametrize("kernel", [False, True])
def test_one_depth_step_loss_and_gradients_match_the_float64_restatement(kernel):
    """tests/test_gpu_trainstep.py::test_one_step_loss_and_gradients_match_the_float64_restatement with the term on (weights 1.0, 1.0; depth
    targets from the sequence's depth maps): loss to 2e-5 relative, every gradient to 2e-3 of the tensor's largest with at most 1e-3 of the
    entries beyond 1e-2 |ref| + 1e-4 max|ref| — that test's bars, set for an L1 + SSIM loss with the same sign discontinuity.
    kernel: the term from das3r_amd.losses.depth_l1 (torch ops) or from das3r_amd.fused.depth_l1_loss (the HIP kernel).
    Tie guard: L1's gradient jumps at D = D*, so pixels where the restatement's |D - D*| < 1e-4 max|D*| leave the mask on BOTH sides; that
    may remove at most 1 % of the pixels (a condition of the test, not a measurement).
    The term must matter: the restatement's xyz gradient with and without it differ by more than ten times the bar."""
    from das3r_amd.fused import depth_l1_loss
    from das3r_amd.losses import depth_l1, depth_l1_weight, l1_loss, psnr, ssim
    from das3r_amd.render import das3r_render
    from das3r_amd.train import depth_term_weight
    model, cams, opt, dense, _seq = _pair(frames=3, W=32, H=24, seed=3, iterations=100)
    bg = torch.zeros(3, device="cuda")
    uid = 1
    cam = cams[uid]
    w = depth_term_weight(cam, opt, 1)
    assert w == depth_l1_weight(opt, 1) == 1.0
    # ---- tie guard from the restatement's float64 D
    with torch.no_grad():
        dense.render(uid, bg.double())
        D64 = dense.invdepth.detach()
    target = cam.invdepthmap
    tie = (D64 - target.double()).abs() < 1e-4 * float(target.abs().max())
    removed = int((tie & (cam.depth_mask > 0)).sum())
    print(f"[tie guard] {removed} of {tie.numel()} pixels removed; D in [{float(D64.min()):.4g}, {float(D64.max()):.4g}], D* in [{float(target.min()):.4g}, {float(target.max()):.4g}]")
    assert removed <= 0.01 * tie.numel(), removed
    mask = (cam.depth_mask * (~tie).float()).contiguous()
    cam.depth_mask = mask
    dense.targets[uid] = (target, mask)
    # ---- the product's step, as train_step composes it
    pkg = das3r_render(cam, model, PIPE, bg, camera_pose=model.get_RT(uid), return_invdepth=True)
    static = model._conf_static[uid]
    image, gt = pkg["render"] * static, cam.original_image * static
    loss = ((1.0 - opt.lambda_dssim) * l1_loss(image, gt, reduce=False) + opt.lambda_dssim * (1.0 - ssim(image, gt, size_average=False))).mean()
    # (as train_step composes it: the kernel form takes the weight into the sweep, so that its gradient is the direct iteration's bit for bit)
    term = depth_l1_loss(pkg["invdepth"], target, mask, static, weight=w) if kernel else w * depth_l1(pkg["invdepth"][0], target, mask, static)
    loss = loss + term
    loss.backward()
    d_loss, d_psnr, d_m2d = dense.loss_of(uid, bg.double())
    d_loss.backward()
    print(f"[loss] product {float(loss):.9g} restatement {float(d_loss):.9g}; weighted depth term {float(term):.6g} vs {w * float(dense.depth_pure):.6g}")
    assert float(dense.depth_pure) > 0.05 * float(d_loss), "the term is a visible part of this loss"
    assert abs(float(loss) - float(d_loss)) <= 2e-5 * abs(float(d_loss)) + 1e-7, (float(loss), float(d_loss))
    assert abs(float(psnr(image, gt).mean()) - float(d_psnr)) < 1e-3
    pairs = [(k, getattr(model, NAMES[k]).grad, dense.p[k].grad) for k in NAMES] + [("means2D", pkg["viewspace_points"].grad, d_m2d.grad)]
    failures = []
    for k, g, r in pairs:
        if k == "f_rest":
            assert (g is None or float(g.abs().max()) == 0.0) and (r is None or float(r.abs().max()) == 0.0)
            continue
        assert g is not None and r is not None, k
        g, r = g.double().reshape(-1), r.reshape(-1)
        scale = float(r.abs().max())
        assert scale > 0, k
        worst = float((g - r).abs().max()) / scale
        bad = float(((g - r).abs() > 1e-2 * r.abs() + 1e-4 * scale).double().mean())
        print(f"[grad {k}] max |g - ref| / max|ref| = {worst:.3g} (bar 2e-3); entries beyond the relative bar {bad:.3g} (bar 1e-3)")
        if worst > 2e-3 or bad > 1e-3:
            failures.append((k, worst, bad))
    assert not failures, failures
    # ---- the term matters here: the restatement's xyz gradient without it
    g_with = dense.p["xyz"].grad.detach().clone()
    dense.opt.zero_grad(set_to_none=True)
    dense.opt_cam.zero_grad(set_to_none=True)
    dense.depth_weight = 0.0
    dense.loss_of(uid, bg.double())[0].backward()
    diff = float((g_with - dense.p["xyz"].grad).abs().max())
    print(f"[term matters] max |d xyz with - without| = {diff:.3g} = {diff / float(g_with.abs().max()):.3g} of the largest gradient (needs > 2e-2)")
    assert diff > 10 * 2e-3 * float(g_with.abs().max())


# ------------------------------------------------------------------------------------------- 7. the three forms agree
FORMS = {"direct-chain": dict(fast_step=True, fuse_geometry_adam=True, fuse_backward_chain=True),
         "direct-no-chain": dict(fast_step=True, fuse_geometry_adam=True, fuse_backward_chain=False),
         "direct-grads": dict(fast_step=True, fuse_geometry_adam=False, fuse_backward_chain=True),
         "autograd-fused": dict(fast_step=False, fuse_geometry_adam=True, fuse_backward_chain=True)}


def _four_steps(form, degree, weights, steps=(0, 2, 1, 0)):
    from das3r_amd import _lib, fast_step
    from das3r_amd.train import train_step
    model, cams, opt, _dense, _seq = _pair(frames=3, W=32, H=24, seed=9, iterations=100, fused=True, weights=weights)
    for k, v in FORMS[form].items():
        setattr(model, k, v)
    assert fast_step.available(model, PIPE) == FORMS[form]["fast_step"]
    model.active_sh_degree = degree
    model.optimizer.set_active_sh_degree(degree)
    with torch.no_grad():
        g = torch.Generator(device="cpu").manual_seed(11)
        model._features_rest.copy_((torch.randn(model._features_rest.shape, generator=g) * 0.05).to(model._features_rest.device))
    bg = torch.zeros(3, device="cuda")
    _lib.forget_shapes()
    _lib.profile_report()
    _lib.profile_enable(True)
    rec = []
    try:
        for it, u in enumerate(steps, start=1):
            loss, ps, pkg = train_step(model, cams[u], opt, it, PIPE, bg, fused=True)
            rec.append((float(loss), float(ps), pkg["viewspace_points"].grad.detach().clone(), int(pkg["visibility_filter"].sum()), "invdepth" in pkg))
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    launches = _depth_launches(_lib.profile_report(raw=True))
    st = model.optimizer.state[model._features_rest]
    return (rec, {k: getattr(model, a).detach().clone() for k, a in NAMES.items()}, st["exp_avg"].clone(), st["step"],
            model.optimizer_cam._gate_state.clone(), launches)


@pytest.mark.parametrize("degree", [0, 1])
def test_direct_chained_unchained_and_autograd_fused_depth_steps_agree(degree):
    """tests/test_gpu_trainstep.py::test_direct_fused_step_matches_the_autograd_fused_step with the term on (weights 1.0 -> 0.5), four steps
    over three cameras: the direct iteration with the backward chained through the pre-transform (das3r_raster_backward_depth with
    grads->chain and in->pre), without the chain, with gradients left on the parameters, and the autograd-fused form — that test's
    tolerances between each direct form and the autograd one.  Kernel profile of the direct forms: per depth step one depth_l1_kernel +
    one depth_l1_finish_kernel (the loss, two launches), one DEPTH forward and no colour-only forward, one depth_pass_inputs_kernel and
    one depth_fold_kernel; the same model with weights 0 runs none of them."""
    out = {form: _four_steps(form, degree, (1.0, 0.5)) for form in FORMS}
    ref = out["autograd-fused"]
    assert all(r[4] for r in ref[0]), "the package of a depth step carries the inverse-depth image"
    failures = []
    for form in ("direct-chain", "direct-no-chain", "direct-grads"):
        (ra, pa, ma, sa, ga, la), (rb, pb, mb, sb, gb, _lb) = out[form], ref
        assert sa == sb == 4 and torch.equal(ga, gb), form
        for step, ((la_, psa, m2a, va, inv), (lb_, psb, m2b, vb, _)) in enumerate(zip(ra, rb), start=1):
            m2 = float((m2a - m2b).abs().max()) / float(m2b.abs().max())
            print(f"[{form} degree {degree} step {step}] loss {la_:.9g} vs {lb_:.9g} (rel {abs(la_ - lb_) / abs(lb_):.3g}), psnr {psa:.7g} vs {psb:.7g}, "
                  f"visible {va} vs {vb}, max |d means2D| difference {m2:.3g} of the largest")
            assert inv
            if not (abs(la_ - lb_) <= 1e-6 * abs(lb_) and abs(psa - psb) <= 1e-4 and va == vb):
                failures.append((form, step, "loss / psnr / visible", la_, lb_, psa, psb, va, vb))
            if not torch.allclose(m2a, m2b, rtol=1e-4, atol=1e-7 * float(m2b.abs().max())):
                failures.append((form, step, "means2D gradient", m2))
        if not torch.allclose(ma, mb, rtol=1e-4, atol=1e-9):
            failures.append((form, "f_rest moments"))
        for k in pa:
            far = float(((pa[k] - pb[k]).abs() > 1e-5 + 1e-4 * pb[k].abs()).double().mean())
            print(f"[{form} degree {degree}] {k}: {far:.3g} of the entries beyond 1e-5 + 1e-4 |ref| (bar 1e-3)")
            if far > 1e-3:
                failures.append((form, k, far))
        assert la == {"depth_l1_kernel": 4, "depth_l1_finish_kernel": 4, "depth_pass_inputs_kernel": 4, "depth_fold_kernel": 4,
                      "depth_forward": 4, "colour_forward": 0}, (form, la)
    # (printed, not asserted: how far the same two forms drift apart over the same four steps WITHOUT the term — the existing test's ground)
    b_dir, b_auto = _four_steps("direct-chain", degree, (0.0, 0.0)), _four_steps("autograd-fused", degree, (0.0, 0.0))
    for step, (x, y) in enumerate(zip(b_dir[0], b_auto[0]), start=1):
        print(f"[photometric only, direct-chain vs autograd-fused, degree {degree} step {step}] loss {x[0]:.9g} vs {y[0]:.9g} (rel {abs(x[0] - y[0]) / abs(y[0]):.3g})")
    assert not failures, failures
    off = _four_steps("direct-chain", degree, (0.0, 0.0))
    assert not any(r[4] for r in off[0])
    assert off[5] == {"depth_l1_kernel": 0, "depth_l1_finish_kernel": 0, "depth_pass_inputs_kernel": 0, "depth_fold_kernel": 0,
                      "depth_forward": 0, "colour_forward": 4}, off[5]
    # the depth term changes the step: the loss of the first step is larger by the weighted term
    assert out["direct-chain"][0][0][0] > off[0][0][0]


# ------------------------------------------------------------------------------------------- 8. inactive is bit-identical
def test_weights_zero_is_the_step_of_a_camera_without_a_depth_target_bit_for_bit():
    """Two models from one seed, six direct fused steps each: cameras that carry invdepthmap / depth_mask with both weights 0 against cameras
    without the attributes.  Every parameter and every Adam moment is torch.equal, the library ran the same kernels (raw names: template
    flags included) the same number of times, and none of them belongs to the depth term."""
    from das3r_amd import _lib, fast_step
    from das3r_amd.train import train_step

    def run(carry):
        model, cams, opt, _dense, _seq = _pair(frames=3, W=32, H=24, seed=9, iterations=100, fused=True, weights=(0.0, 0.0), carry=carry)
        assert all(hasattr(c, "invdepthmap") == carry for c in cams) and fast_step.available(model, PIPE)
        bg = torch.zeros(3, device="cuda")
        _lib.forget_shapes()
        _lib.profile_report()
        _lib.profile_enable(True)
        try:
            losses = [float(train_step(model, cams[u], opt, it, PIPE, bg, fused=True)[0]) for it, u in enumerate([0, 2, 1, 0, 1, 2], start=1)]
            torch.cuda.synchronize()
        finally:
            _lib.profile_enable(False)
        kernels = {k: n for k, (n, _ms) in _lib.profile_report(raw=True).items()}
        moments = {}
        for name, o in (("optimizer", model.optimizer), ("optimizer_cam", model.optimizer_cam)):
            for gi, g in enumerate(o.param_groups):
                for p in g["params"]:
                    st = o.state.get(p)
                    if st is not None:
                        moments[(name, g.get("name", gi))] = (st["step"], st["exp_avg"].clone(), st["exp_avg_sq"].clone())
        return losses, {k: getattr(model, a).detach().clone() for k, a in NAMES.items()}, moments, kernels

    (la, pa, ma, ka), (lb, pb, mb, kb) = run(True), run(False)
    assert la == lb
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert set(ma) == set(mb) and len(ma) >= 8
    for k in ma:
        assert ma[k][0] == mb[k][0] and torch.equal(ma[k][1], mb[k][1]) and torch.equal(ma[k][2], mb[k][2]), k
    assert ka == kb, (ka, kb)
    launches = _depth_launches({k: (n, 0.0) for k, n in ka.items()})
    assert launches.pop("colour_forward") == 6 and not any(launches.values()), launches


# ------------------------------------------------------------------------------------------- 9. schedule end to end
def _median_depth_l1(model, cams):
    from das3r_amd.losses import depth_l1
    from das3r_amd.render import das3r_render
    bg = torch.zeros(3, device="cuda")
    vals = []
    with torch.no_grad():
        for c in cams:
            pkg = das3r_render(c, model, PIPE, bg, camera_pose=model.get_RT(c.uid), fused=True, return_invdepth=True)
            vals.append(float(depth_l1(pkg["invdepth"][0].double(), c.invdepthmap.double(), c.depth_mask.double(), model._conf_static[c.uid].double())))
    return float(np.median(vals))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_depth_supervision_lowers_the_depth_error_of_a_trained_model(seed):
    """consistent_sequence (8 frames, 128 x 48, a small cloud, exact depth maps, nothing moving), 300 fused iterations twice from one seed:
    weights (1.0, 0.01) against (0, 0).  The median over the training views of L_depth_pure after training must be lower with the term."""
    from das3r_amd import _lib
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, consistent_sequence, train
    seq = consistent_sequence(frames=8, W=128, H=48, focal=150.0, n_splats=3000, seed=seed, moving=False, depth_noise=0.0)
    res = {}
    for name, (w0, w1) in (("with", (1.0, 0.01)), ("without", (0.0, 0.0))):
        model, cams = build_from_sequence(copy.deepcopy(seq), depth_targets=True)
        opt = OptimParams(iterations=300, depth_l1_weight_init=w0, depth_l1_weight_final=w1)
        model.training_setup(opt, fused=True)
        _lib.forget_shapes()
        before = _median_depth_l1(model, cams)
        stats = train(model, cams, opt, 300, pipe=PIPE, seed=seed, fused=True)
        res[name] = (_median_depth_l1(model, cams), stats["psnr"], before)
    print(f"[schedule seed {seed}] median L_depth_pure before {res['with'][2]:.6g}; after 300 iterations with the term {res['with'][0]:.6g} "
          f"(last frame PSNR {res['with'][1]:.3f} dB), without {res['without'][0]:.6g} ({res['without'][1]:.3f} dB)")
    assert res["with"][0] < res["without"][0], res


# ------------------------------------------------------------------------------------------- 10. resume
SMALL = dict(frames=12, W=256, H=104, focal=300.0, n_splats=8000)


def test_depth_supervised_job_resumes_bit_identical_and_refuses_other_weights(tmp_path):
    """tests/test_gpu_resume_offline.py's resume test with depth supervision on: a job of 90 iterations that checkpoints every 30, and the
    same job killed after iteration 60 and resumed, end with EQUAL parameters (the schedule's weight at iteration 61.. is the uninterrupted
    job's).  The weights are in the checkpoint's extras; resuming with other weights raises instead of changing the schedule."""
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.train import ResumeMismatch, consistent_sequence, latest_checkpoint
    dev = torch.device("cuda:0")
    seq = consistent_sequence(seed=5, **SMALL)
    full_dir, res_dir, bad_dir = str(tmp_path / "full"), str(tmp_path / "resumed"), str(tmp_path / "other")
    keep_full, keep_res, keep_plain = {}, {}, {}
    kw = dict(fused=True, seq=seq, checkpoint_every=30, depth_l1_init=1.0, depth_l1_final=0.01)
    full = run_sequence_job(3, 90, dev, out_dir=full_dir, keep=keep_full, **kw)
    assert full["ok"] == 1 and latest_checkpoint(full_dir)[1] == 60
    extras = torch.load(os.path.join(full_dir, "chkpnt60.das3r.pth"), weights_only=False)
    assert tuple(extras["loop"]["depth_l1"]) == (1.0, 0.01)
    for d in (res_dir, bad_dir):
        os.makedirs(d)
        for f in ("chkpnt60.pth", "chkpnt60.das3r.pth"):
            shutil.copy(os.path.join(full_dir, f), os.path.join(d, f))
    res = run_sequence_job(3, 90, dev, out_dir=res_dir, resume=True, keep=keep_res, **kw)
    assert res["ok"] == 1
    a, b = keep_full[3][0], keep_res[3][0]
    assert a is not b and all(hasattr(c, "invdepthmap") for c in keep_res[3][1]) and not any(hasattr(c, "invdepthmap") for c in keep_res[3][2])
    for n in NAMES.values():
        assert torch.equal(getattr(a, n).detach(), getattr(b, n).detach()), f"{n}: a resumed depth-supervised job must end bit-identical"
    assert res["psnr"] == full["psnr"]
    # the term was on: the same job without it ends elsewhere
    plain = run_sequence_job(3, 90, dev, fused=True, seq=seq, keep=keep_plain)
    assert plain["ok"] == 1 and not torch.equal(keep_plain[3][0]._xyz.detach(), a._xyz.detach())
    with pytest.raises(ResumeMismatch, match="depth-l1"):
        run_sequence_job(3, 90, dev, out_dir=bad_dir, resume=True, fused=True, seq=seq, checkpoint_every=30, depth_l1_init=1.0, depth_l1_final=0.1)
    with pytest.raises(ResumeMismatch):
        run_sequence_job(3, 90, dev, out_dir=bad_dir, resume=True, fused=True, seq=seq, checkpoint_every=30)
