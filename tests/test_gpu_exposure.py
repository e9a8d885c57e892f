"""GPU tests of per-frame exposure compensation (INTEGRATION.md "Exposure compensation"): the two loss kernels with E applied inside and the
reduction of dL/dE against losses.apply_exposure + the torch loss in float64; [I | 0] with the learning rate held at 0 against the step
without the feature, bit for bit; the switched-off step's kernels; the plain, autograd-fused and direct forms against each other; the one
launch the feature adds; the flicker experiment end to end; resume and pruning."""
import copy
import ctypes as C
import importlib.util
import os
import shutil
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_conf_static", "Q", "T")
RATES = (0.01, 0.001)   # upstream's
EXPOSURE_KERNELS = ("photometric_forward_exposure_kernel", "photometric_backward_exposure_kernel", "exposure_grad_finish_kernel")


def _tool(name):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", name + ".py")
    spec = importlib.util.spec_from_file_location("das3r_tool_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------------------- 1. kernel parity
def _kernel_run(render, gt, static, E, lam):
    from das3r_amd.fused import masked_photometric_loss
    r, s, e = render.clone().requires_grad_(True), static.clone().requires_grad_(True), E.clone().requires_grad_(True)
    loss, mse = masked_photometric_loss(r, gt, s, lam, exposure=e)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), mse.detach(), r.grad, s.grad, e.grad


@pytest.mark.parametrize("hw", [(16, 16), (37, 53), (208, 512)])
def test_exposure_kernels_match_apply_exposure_and_the_torch_loss_in_float64(hw):
    """Random render / ground truth / static map, E = [I | 0] + N(0, 0.1), lambda 0.2.  Reference: losses.apply_exposure followed by the torch
    loss of das3r_amd.losses, in float64.  Loss and MSE to 2e-6 relative, the gradients of the render and the static map to 2e-5 of their
    maximum (the bars tests/test_gpu_fused.py holds the photometric kernels to: the new code adds 12 FMAs per pixel); each of the twelve
    exposure gradients to 2e-5 of the sum over the pixels of |its terms| (taken here in float64: every term carries the per-pixel
    tolerance, the ordered tree sum adds a few ulps); two runs bit-identical."""
    from das3r_amd.losses import apply_exposure, l1_loss, ssim
    H, W = hw
    lam = 0.2
    g = torch.Generator().manual_seed(H * 1013 + W)
    render, gt = torch.rand(3, H, W, generator=g).cuda(), torch.rand(3, H, W, generator=g).cuda()
    static = (0.2 + 0.8 * torch.rand(H, W, generator=g)).cuda()
    E = (torch.eye(3, 4) + 0.1 * torch.randn(3, 4, generator=g)).cuda()
    loss_a, mse_a, gr_a, gs_a, ge_a = _kernel_run(render, gt, static, E, lam)
    loss_b, mse_b, gr_b, gs_b, ge_b = _kernel_run(render, gt, static, E, lam)
    for x, y in ((loss_a, loss_b), (mse_a, mse_b), (gr_a, gr_b), (gs_a, gs_b), (ge_a, ge_b)):
        assert torch.equal(x, y), "two runs must be bit-identical"
    # ---- the float64 reference
    r64, s64, e64 = (t.double().clone().requires_grad_(True) for t in (render, static, E))
    image = apply_exposure(r64, e64) * s64
    image.retain_grad()
    target = gt.double() * s64
    loss_t = ((1.0 - lam) * l1_loss(image, target, reduce=False) + lam * (1.0 - ssim(image, target, size_average=False))).mean()
    mse_t = ((image - target) ** 2).reshape(3, -1).mean(1).detach()
    loss_t.backward()
    rel = abs(float(loss_a) - float(loss_t)) / abs(float(loss_t))
    mse_rel = float((mse_a.double() - mse_t).abs().max()) / float(mse_t.abs().max())
    print(f"[{H}x{W}] loss {float(loss_a):.9g} vs float64 {float(loss_t):.9g}: rel {rel:.3g} (bar 2e-6); mse rel {mse_rel:.3g} (bar 2e-6)")
    failures = []
    if rel > 2e-6 or mse_rel > 2e-6:
        failures.append(("loss / mse", rel, mse_rel))
    for name, got, ref in (("render", gr_a, r64.grad), ("static", gs_a, s64.grad)):
        worst = float((got.double() - ref).abs().max()) / float(ref.abs().max())
        print(f"[{H}x{W}] d {name}: max |g - ref| / max|ref| = {worst:.3g} (bar 2e-5)")
        if worst > 2e-5:
            failures.append((name, worst))
    # ---- dL/dE: term sums in float64; the bar of each is 2e-5 of the sum of |terms|
    gimg = image.grad.detach()                                                   # g_c(p)
    gs = gimg * s64.detach()                                                     # g_c(p) static(p)
    bars = torch.zeros(3, 4, dtype=torch.float64, device="cuda")
    for i in range(3):
        for c in range(3):
            bars[i, c] = (gs[c] * r64.detach()[i]).abs().sum()
    for c in range(3):
        bars[c, 3] = gs[c].abs().sum()
    err = (ge_a.double() - e64.grad).abs()
    ratio = err / bars
    print(f"[{H}x{W}] dL/dE: max |g - ref| / sum|terms| = {float(ratio.max()):.3g} (bar 2e-5); |ref| / sum|terms| in "
          f"[{float((e64.grad.abs() / bars).min()):.3g}, {float((e64.grad.abs() / bars).max()):.3g}]")
    if bool((err > 2e-5 * bars).any()):
        failures.append(("exposure", ratio.tolist()))
    assert not failures, failures


def test_exposure_grad_finish_zeroes_the_previous_row_before_it_writes():
    """das3r_exposure_grad_finish in the pattern of das3r_pose_chain_qt_rearm: the row another view left is zeroed, this view's row written,
    every other row untouched; the row to zero may be the row to write; the sum is the rows of epartials (columns 12..15 are not read into
    the result)."""
    from das3r_amd import _lib
    lib = _lib.load()
    H, W = 37, 53
    nb = int(lib.das3r_photometric_blocks(H, W))
    g = torch.Generator().manual_seed(5)
    ep = torch.randn(nb, 16, generator=g).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.full((5, 3, 4), 9.0, device="cuda")
    _lib.check(lib.das3r_exposure_grad_finish(H, W, p(ep), p(buf[2]), p(buf[4]), s), "finish")
    torch.cuda.synchronize()
    want = ep[:, :12].double().sum(0).reshape(3, 4)
    assert float((buf[2].double() - want).abs().max()) <= 1e-5 * float(ep.abs().sum(0).max())
    assert float(buf[4].abs().max()) == 0.0 and float(buf[[0, 1, 3]].min()) == 9.0
    first = buf[2].clone()
    _lib.check(lib.das3r_exposure_grad_finish(H, W, p(ep), p(buf[2]), p(buf[2]), s), "finish, same row")
    torch.cuda.synchronize()
    assert torch.equal(buf[2], first)


@pytest.mark.parametrize("hw", [(16, 16), (37, 53), (208, 512)])
def test_exposure_kernels_with_the_identity_matrix_give_the_plain_kernels_bits(hw):
    """E = [I | 0] handed to das3r_photometric_forward_exposure / _backward_finish_exposure against das3r_photometric_forward /
    _backward_finish on the same random inputs: the tile sums, the derivative maps, out8, d_render and d_static are torch.equal (an FMA
    chain with exact ones and zeros returns r_c exactly, and the exposure backward does the plain form's arithmetic operation for
    operation); dL/dE comes out finite beside them."""
    from das3r_amd import _lib
    lib = _lib.load()
    H, W = hw
    g = torch.Generator().manual_seed(H * 211 + W)
    render, gt = torch.rand(3, H, W, generator=g).cuda(), torch.rand(3, H, W, generator=g).cuda()
    static = (0.2 + 0.8 * torch.rand(H, W, generator=g)).cuda()
    static[: H // 3, : W // 4] = 0.0   # (a masked region, as the moving object leaves one)
    E = torch.eye(3, 4, device="cuda").contiguous()
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = int(lib.das3r_photometric_blocks(H, W))
    lam, one = C.c_float(0.2), torch.ones(1, device="cuda")
    mk = lambda: (torch.zeros(nb, 8, device="cuda"), torch.zeros(4, 3, H, W, device="cuda"), torch.zeros(8, device="cuda"),
                  torch.zeros_like(render), torch.zeros(H, W, device="cuda"))
    pa, dm_a, o_a, dr_a, ds_a = mk()
    pb, dm_b, o_b, dr_b, ds_b = mk()
    ep, ge = torch.zeros(nb, 16, device="cuda"), torch.zeros(3, 4, device="cuda")
    _lib.check(lib.das3r_photometric_forward(H, W, p(render), p(gt), p(static), lam, p(pa), p(dm_a), s), "forward")
    _lib.check(lib.das3r_photometric_backward_finish(H, W, p(render), p(gt), p(static), lam, p(dm_a), p(one), p(dr_a), p(ds_a), p(pa), p(o_a), s), "backward")
    _lib.check(lib.das3r_photometric_forward_exposure(H, W, p(render), p(gt), p(static), lam, p(E), p(pb), p(dm_b), s), "forward, exposure")
    _lib.check(lib.das3r_photometric_backward_finish_exposure(H, W, p(render), p(gt), p(static), lam, p(E), p(dm_b), p(one), p(dr_b), p(ds_b), p(pb),
                                                              p(o_b), p(ep), s), "backward, exposure")
    _lib.check(lib.das3r_exposure_grad_finish(H, W, p(ep), p(ge), None, s), "finish")
    torch.cuda.synchronize()
    for name, x, y in (("partials", pa[:, :5], pb[:, :5]), ("dmaps", dm_a, dm_b), ("out8", o_a[:5], o_b[:5]), ("d_render", dr_a, dr_b),
                       ("d_static", ds_a, ds_b)):
        diff = int((x != y).sum())
        print(f"[{H}x{W}] {name}: {diff} of {x.numel()} elements differ")
        assert torch.equal(x, y), name
    assert torch.isfinite(ge).all() and float(ge.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ models for the step tests
def _model(rates, fused=True, seed=2, generic=True, perturb_E=0.0, frames=3, W=96, H=64):
    """tests/test_gpu_fused.py::test_train_step_fused_matches_default's scene and generic state; rates: the exposure learning rates."""
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    seq = synthetic_sequence(frames=frames, W=W, H=H, focal=90.0, n_splats=3000, seed=seed)
    model, cams = build_from_sequence(copy.deepcopy(seq))
    if generic:
        gen = torch.Generator().manual_seed(7)
        with torch.no_grad():
            model._scaling += 0.4 * torch.randn(model._scaling.shape, generator=gen).cuda()
            model._rotation.copy_(torch.nn.functional.normalize(torch.randn(model._rotation.shape, generator=gen)).cuda())
    opt = OptimParams(iterations=100, psnr_threshold=0.0, exposure_lr_init=rates[0], exposure_lr_final=rates[1])
    model.training_setup(opt, fused=fused)
    if perturb_E and model._exposure is not None:
        gen = torch.Generator().manual_seed(11)
        with torch.no_grad():
            model._exposure += (perturb_E * torch.randn(model._exposure.shape, generator=gen)).cuda()
    return model, cams, opt


def _steps(model, cams, opt, order=(1, 2, 0), fused=True, profile=False):
    from das3r_amd import _lib
    from das3r_amd.train import train_step
    bg = torch.zeros(3, device="cuda")
    _lib.forget_shapes()
    if profile:
        _lib.profile_report()
        _lib.profile_enable(True)
    rec = []
    try:
        for it, u in enumerate(order, start=1):
            loss, ps, pkg = train_step(model, cams[u], opt, it, PIPE, bg, fused=fused)
            rec.append((float(loss), float(ps)))
        torch.cuda.synchronize()
    finally:
        if profile:
            _lib.profile_enable(False)
    return rec, ({k: n for k, (n, _ms) in _lib.profile_report(raw=True).items()} if profile else None)


# ---------------------------------------------------------------------------------------------------------------- 2. identity is free of effect
def test_identity_with_the_learning_rate_at_zero_is_the_step_without_the_feature_bit_for_bit():
    """The feature on, its learning rate held at 0 (the schedule replaced after training_setup: with both OptimParams rates 0 the feature
    would be off): the kernels' input stays [I | 0], an FMA chain with exact ones and zeros returns r_c exactly, and loss, psnr_frame and
    every parameter after three direct steps equal those of the step without the feature."""
    from das3r_amd import fast_step
    on, cams_on, opt_on = _model(RATES)
    on._lr_exposure = lambda iteration: 0.0
    off, cams_off, opt_off = _model((0.0, 0.0))
    assert fast_step.available(on, PIPE) and fast_step.available(off, PIPE) and on._exposure is not None and off._exposure is None
    rec_on, k_on = _steps(on, cams_on, opt_on, profile=True)
    rec_off, _ = _steps(off, cams_off, opt_off)
    assert k_on["exposure_grad_finish_kernel"] == 3, "the exposure kernels did run"
    assert rec_on == rec_off, (rec_on, rec_off)
    for n in NAMES:
        assert torch.equal(getattr(on, n).detach(), getattr(off, n).detach()), n
    assert torch.equal(on._exposure.detach(), torch.eye(3, 4, device="cuda")[None].repeat(3, 1, 1)), "a step with lr 0 leaves [I | 0]"
    st = on.optimizer.state[on._exposure]
    assert st["step"] == 3 and float(st["exp_avg"].abs().max()) > 0, "the group did step (moments moved), with lr 0"


# ---------------------------------------------------------------------------------------------------------------- 3. off is today's step
def test_with_the_defaults_no_exposure_kernel_runs_and_no_parameter_exists():
    """The depth test's weights-zero check for this feature: with the default OptimParams the library profiler's kernel names (raw: template
    flags included) are those of a photometric step — per step one photometric_forward_kernel and one photometric_backward_kernel, nothing
    whose name holds "exposure" — no _exposure exists, the optimizer has its seven groups, and the direct step's state holds no exposure
    gradient buffer."""
    model, cams, opt = _model((0.0, 0.0))
    rec, kernels = _steps(model, cams, opt, order=(1, 2, 0, 1), profile=True)
    assert model._exposure is None and len(model.optimizer.param_groups) == 7 and model._fast_state.Eg is None
    assert not [k for k in kernels if "exposure" in k], kernels
    assert kernels["photometric_forward_kernel"] == 4 and kernels["photometric_backward_kernel"] == 4
    assert kernels["pose_chain_kernel"] == 4


# ---------------------------------------------------------------------------------------------------------------- 4. the three paths agree
FORMS = {"plain": dict(fused=False),
         "autograd-fused": dict(fused=True, fast_step=False),
         "direct-chain": dict(fused=True, fast_step=True, fuse_backward_chain=True),
         "direct-no-chain": dict(fused=True, fast_step=True, fuse_backward_chain=False)}


def test_plain_autograd_fused_and_direct_exposure_steps_agree():
    """Three steps from the generic state of tests/test_gpu_fused.py::test_train_step_fused_matches_default with the exposure group stepping
    (rates 0.01 -> 0.001; the matrices start at [I | 0] + N(0, 0.05) so that every entry mixes): plain autograd (torch ops, torch.optim.Adam),
    autograd-fused, and the direct form with and without the chained backward.  That test's tolerances against the plain form: losses to
    1e-5 relative; per tensor at most 5e-3 of the entries beyond 2e-4 max|ref| + 1e-6 — _exposure among the tensors."""
    from das3r_amd import fast_step
    out = {}
    for form, cfg in FORMS.items():
        cfg = dict(cfg)
        fused = cfg.pop("fused")
        model, cams, opt = _model(RATES, fused=fused, perturb_E=0.05)
        for k, v in cfg.items():
            setattr(model, k, v)
        if fused:
            assert fast_step.available(model, PIPE) == cfg["fast_step"]
        rec, _ = _steps(model, cams, opt, fused=fused)
        out[form] = (rec, {n: getattr(model, n).detach().clone() for n in NAMES + ("_exposure",)})
    ref_rec, ref_p = out["plain"]
    start = torch.eye(3, 4, device="cuda")
    assert float((ref_p["_exposure"] - start).abs().max()) > 0.02, "the group stepped"
    failures = []
    for form in ("autograd-fused", "direct-chain", "direct-no-chain"):
        rec, p = out[form]
        for step, ((la, pa), (lb, pb)) in enumerate(zip(rec, ref_rec), start=1):
            print(f"[{form} step {step}] loss {la:.9g} vs plain {lb:.9g} (rel {abs(la - lb) / abs(lb):.3g}), psnr_frame {pa:.7g} vs {pb:.7g}")
            if abs(la - lb) > 1e-5 * max(abs(lb), 1e-3):
                failures.append((form, step, la, lb))
        for n in p:
            tol = 2e-4 * float(ref_p[n].abs().max()) + 1e-6
            far = float(((p[n] - ref_p[n]).abs() > tol).float().mean())
            print(f"[{form}] {n}: {far:.3g} of the entries beyond {tol:.3g} (bar 5e-3); max |difference| {float((p[n] - ref_p[n]).abs().max()):.3g}")
            if far > 5e-3:
                failures.append((form, n, far))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------- 5. launch count
def test_an_exposure_step_launches_at_most_one_kernel_more():
    """Counted with the library's profiler over four direct steps: the exposure step runs the two loss kernels in their exposure form in
    place of the plain ones and exposure_grad_finish_kernel besides — one launch more per step, and the exposure group rides in the
    optimizer's one launch (no further adam launch)."""
    on, cams_on, opt_on = _model(RATES)
    off, cams_off, opt_off = _model((0.0, 0.0))
    _, k_on = _steps(on, cams_on, opt_on, order=(1, 2, 0, 1), profile=True)
    _, k_off = _steps(off, cams_off, opt_off, order=(1, 2, 0, 1), profile=True)
    n_on, n_off = sum(k_on.values()), sum(k_off.values())
    print(f"launches over four steps: {n_on} with exposure, {n_off} without; exposure kernels {[(k, k_on.get(k, 0)) for k in EXPOSURE_KERNELS]}")
    assert n_on <= n_off + 4, (k_on, k_off)
    assert [k_on.get(k, 0) for k in EXPOSURE_KERNELS] == [4, 4, 4]
    assert "photometric_forward_kernel" not in k_on and "photometric_backward_kernel" not in k_on
    rest_on = {k: v for k, v in k_on.items() if k not in EXPOSURE_KERNELS}
    rest_off = {k: v for k, v in k_off.items() if k not in ("photometric_forward_kernel", "photometric_backward_kernel")}
    assert rest_on == rest_off, (rest_on, rest_off)


# ---------------------------------------------------------------------------------------------------------------- 6. it does its job
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_exposure_compensation_explains_the_flicker_of_a_trained_sequence(seed):
    """tools/exposure_quality.py's measurement (consistent_sequence + apply_flicker; 600 fused iterations — the depth term's end-to-end test
    trains 300 — with the feature at 0.01 -> 0.001 and without, from one seed).  Two orderings, per seed, no thresholds:
    (a) the median training-view PSNR of the compensated render against the flickered frames is higher with the feature than without;
    (b) the learned per-channel log-gains (diagonal of E_f, centred over the frames) are closer to the applied ones, as a mean absolute
        difference, than all-zero log-gains are.
    The held-out PSNR under both policies is printed, not asserted: nothing pins the global colour scale."""
    tool = _tool("exposure_quality")
    assert tool.ITERATIONS == 600
    row = tool.measure(seed, tool.ITERATIONS)
    w, wo = row["with"], row["without"]
    print(f"[flicker seed {seed}] median training-view PSNR {w['median_train_psnr']:.3f} dB with, {wo['median_train_psnr']:.3f} dB without; "
          f"log-gain MAD {w['log_gain_mad']:.4f} (identity: {w['log_gain_mad_of_identity']:.4f}); held-out PSNR with: identity "
          f"{w['heldout_psnr_identity']:.3f}, nearest {w['heldout_psnr_nearest']:.3f}; without: {wo['heldout_psnr_identity']:.3f}")
    assert wo["heldout_psnr_identity"] == wo["heldout_psnr_nearest"], "without matrices both policies are the raw render"
    assert w["median_train_psnr"] > wo["median_train_psnr"], row
    assert w["log_gain_mad"] < w["log_gain_mad_of_identity"], row


# ---------------------------------------------------------------------------------------------------------------- 7. resume and pruning
SMALL = dict(frames=12, W=256, H=104, focal=300.0, n_splats=8000)


def test_exposure_job_resumes_bit_identical_writes_exposure_json_and_refuses_other_rates(tmp_path):
    """tests/test_gpu_depth_train.py's resume test with exposure compensation on (flickered frames, the "nearest" held-out policy): a job of
    90 iterations that checkpoints every 30 and the same job killed after iteration 60 and resumed end with EQUAL parameters, matrices and
    moments; both write the same exposure.json; resuming with other rates — or none — raises."""
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.io_formats import read_exposure_json
    from das3r_amd.train import ResumeMismatch, apply_flicker, consistent_sequence, latest_checkpoint
    dev = torch.device("cuda:0")
    seq = consistent_sequence(seed=5, **SMALL)
    apply_flicker(seq, 5)
    full_dir, res_dir, bad_dir = str(tmp_path / "full"), str(tmp_path / "resumed"), str(tmp_path / "other")
    keep_full, keep_res = {}, {}
    kw = dict(fused=True, seq=seq, checkpoint_every=30, exposure_lr_init=0.01, exposure_lr_final=0.001, exposure_heldout="nearest")
    full = run_sequence_job(3, 90, dev, out_dir=full_dir, keep=keep_full, **kw)
    assert full["ok"] == 1 and latest_checkpoint(full_dir)[1] == 60
    extras = torch.load(os.path.join(full_dir, "chkpnt60.das3r.pth"), weights_only=False)
    assert tuple(extras["loop"]["exposure"]) == (0.01, 0.001) and tuple(extras["model"]["exposure"].shape) == (11, 3, 4)
    for d in (res_dir, bad_dir):
        os.makedirs(d)
        for f in ("chkpnt60.pth", "chkpnt60.das3r.pth"):
            shutil.copy(os.path.join(full_dir, f), os.path.join(d, f))
    res = run_sequence_job(3, 90, dev, out_dir=res_dir, resume=True, keep=keep_res, **kw)
    assert res["ok"] == 1
    a, b = keep_full[3][0], keep_res[3][0]
    assert a is not b
    for n in NAMES + ("_exposure",):
        assert torch.equal(getattr(a, n).detach(), getattr(b, n).detach()), f"{n}: a resumed exposure job must end bit-identical"
    sa, sb = a.optimizer.state[a._exposure], b.optimizer.state[b._exposure]
    assert sa["step"] == sb["step"] == 90 and torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    assert res["psnr"] == full["psnr"]
    assert float((a._exposure.detach() - torch.eye(3, 4, device=dev)).abs().max()) > 0.01, "the matrices were learnt"
    ja, jb = read_exposure_json(os.path.join(full_dir, "exposure.json")), read_exposure_json(os.path.join(res_dir, "exposure.json"))
    names = [f"frame_{i:04d}.png" for i in range(12) if i != 5]
    assert list(ja) == names == list(jb)
    for k, n in enumerate(names):
        assert (ja[n] == a._exposure.detach()[k].cpu().numpy()).all() and (ja[n] == jb[n]).all(), n
    with pytest.raises(ResumeMismatch, match="exposure-lr"):
        run_sequence_job(3, 90, dev, out_dir=bad_dir, resume=True, fused=True, seq=seq, checkpoint_every=30, exposure_lr_init=0.01, exposure_lr_final=0.01)
    with pytest.raises(ResumeMismatch):
        run_sequence_job(3, 90, dev, out_dir=bad_dir, resume=True, fused=True, seq=seq, checkpoint_every=30)


def test_a_prune_event_leaves_the_matrices_and_their_moments_and_the_next_step_runs():
    from das3r_amd.prune import prune_points
    from das3r_amd.train import train_step
    model, cams, opt = _model(RATES, generic=False)
    bg = torch.zeros(3, device="cuda")
    for it, u in enumerate((0, 1, 2), start=1):
        train_step(model, cams[u], opt, it, PIPE, bg, fused=True)
    E = model._exposure
    before = E.detach().clone()
    st = model.optimizer.state[E]
    moments = (st["step"], st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    P = model._xyz.shape[0]
    also = torch.zeros(P, dtype=torch.bool, device="cuda")
    also[::4] = True
    info = prune_points(model, min_opacity=0.005, also_drop=also)
    assert info["dropped"] >= P // 4 and model._xyz.shape[0] == info["after"]
    assert model._exposure is E and torch.equal(E.detach(), before) and model.optimizer.param_groups[7]["params"][0] is E
    st = model.optimizer.state[E]
    assert st["step"] == moments[0] and torch.equal(st["exp_avg"], moments[1]) and torch.equal(st["exp_avg_sq"], moments[2])
    loss, ps, _ = train_step(model, cams[1], opt, 4, PIPE, bg, fused=True)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(ps) and model.optimizer.state[E]["step"] == 4
    assert not torch.equal(E.detach(), before) and torch.isfinite(E).all()


# ---------------------------------------------------------------------------------------------------------------- the held-out pass
def test_the_heldout_pose_pass_takes_no_exposure_gradient_and_steps_nothing():
    """Both held-out policies, direct and autograd-fused: after a pass over the held-out views no parameter has changed, the exposure group's
    step count stands, _exposure carries no gradient, and exposure_grad_finish_kernel did not run."""
    import random
    from das3r_amd import _lib
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, synthetic_sequence, test_pose_pass, train_step
    seq = synthetic_sequence(frames=8, W=96, H=64, focal=90.0, n_splats=3000, seed=2)
    for direct in (True, False):
        model, cams, test = build_from_sequence(copy.deepcopy(seq), heldout=True)
        opt = OptimParams(iterations=100, psnr_threshold=0.0, exposure_lr_init=0.01, exposure_lr_final=0.001)
        model.training_setup(opt, fused=True)
        model.fast_step = direct
        bg = torch.zeros(3, device="cuda")
        for it in (1, 2):
            train_step(model, cams[it], opt, it, PIPE, bg, fused=True)
        snap = {n: getattr(model, n).detach().clone() for n in NAMES + ("_exposure",)}
        for policy in ("identity", "nearest"):
            _lib.profile_report()
            _lib.profile_enable(True)
            try:
                test_pose_pass(model, test, None, opt, PIPE, bg, random.Random(0), fused=True, exposure=policy)
                torch.cuda.synchronize()
            finally:
                _lib.profile_enable(False)
            kernels = _lib.profile_report(raw=True)
            assert "exposure_grad_finish_kernel" not in kernels, (direct, policy)
            assert ("photometric_forward_exposure_kernel" in kernels) == (policy == "nearest"), (direct, policy, sorted(kernels))
            assert model._exposure.grad is None and model.optimizer.state[model._exposure]["step"] == 2
            for n, v in snap.items():
                assert torch.equal(getattr(model, n).detach(), v), (direct, policy, n)
