"""GPU tests of the focal gradient (das3r_raster_backward_focal, das3r_amd/csrc/focal_grad.hip) and of the trainable field of view built
on it (GaussianRasterizer(...)(..., log_focal=...), OptimParams.fov_lr).

The reference is tests/focal_reference.py: every splat's own dL/d(log-focal offsets) from the unchanged float64 dense oracle, which
tests/test_focal_host.py holds to central differences of the true field-of-view change.  The kernel's per_splat output is held to it at
the bar of every other per-Gaussian gradient (util.GRAD_REL_TOL of the tensor's maximum, threshold flips named)."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from tests import focal_reference as fr
from tests import util

pytestmark = pytest.mark.gpu

PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
VARIANTS = ["basic_deg3", "deg0", "ragged_image", "colors_precomp", "cov3D_precomp", "scale_modifier", "long_lists", "deep", "world_camera",
            "culled", "depth_ties", "single"] + util.CAMERA_VARIANTS
GRAD_NAMES = ["means2D", "colors", "opacities", "means3D", "cov3D", "shs", "scales", "rotations"]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _scene(name):
    """util.scene_variant, plus tests/test_gpu_antialiasing.py's "aa_tiny" (splats from well below a pixel to a few pixels: the clamp of rho)."""
    if name != "aa_tiny":
        return util.scene_variant(name)
    from das3r_amd.synth import make_scene
    sc = make_scene(P=1500, W=96, H=64, focal=80.0, sh_degree=2, seed=41, s_px=(0.01, 4.0), bg=(0.1, 0.2, 0.3))
    sc.opacities[: sc.P // 2] = 0.99
    return sc, dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)


def _g_depth(sc):
    return torch.randn(sc.H, sc.W, generator=torch.Generator().manual_seed(5)) * 0.5


@functools.lru_cache(maxsize=None)
def _reference(name, depth=False, aa=False):
    """(c [P, 2] float64 on the host, sum |c_i| per axis): computed once per (scene, mode), shared and never written."""
    sc, mode = _scene(name)
    c, _ = fr.per_splat(sc, mode, _dev(), g_depth=_g_depth(sc) if depth else None, aa=aa)
    c = c.cpu()
    return c, c.abs().sum(0)


def _pre_of(sc, dev, keep):
    """The raw-parameter form (das3r_raster_in.pre) of the scene: identity pose, log scales, opacity logits with confidence 1."""
    from das3r_amd import _lib
    xyz, rot = sc.means3D.to(dev), sc.rotations.to(dev)
    scaling = torch.log(sc.scales).to(dev)
    op = sc.opacities.clamp(1e-4, 1 - 1e-4)
    logit = torch.log(op / (1 - op)).to(dev)
    conf = torch.ones(sc.P, device=dev)
    mats = torch.zeros(28, device=dev)
    mats[[0, 4, 8]] = 1.0
    mats[[12, 17, 22, 27]] = 1.0
    keep += [xyz, rot, scaling, logit, conf, mats]
    pre = _lib.PreTransform()
    pre.xyz, pre.rot, pre.scaling, pre.opacity_raw = xyz.data_ptr(), rot.data_ptr(), scaling.data_ptr(), logit.data_ptr()
    pre.conf_flat, pre.mask_index = conf.data_ptr(), None
    pre.R, pre.t, pre.Lq = mats.data_ptr(), mats.data_ptr() + 36, mats.data_ptr() + 48
    return pre


class _Call:
    """One forward of a scene through rasterizer._forward_full; backward(...) runs das3r_raster_backward[_depth | _focal] on it any number of times."""

    def __init__(self, name, depth=False, aa=False, use_pre=False, sh_cols=None):
        from das3r_amd import GaussianRasterizationSettings, rasterizer
        self.sc, self.mode = _scene(name)
        sc, mode, dev = self.sc, self.mode, _dev()
        self.dev = dev
        kw = {k: v.to(dev) for k, v in util.raster_inputs(sc, mode).items()}
        if sh_cols is not None:
            kw["shs"] = kw["shs"][:, :sh_cols].contiguous()
        self.rs = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()})
        e = torch.empty(0, device=dev)
        self.keep = []
        self.pre = _pre_of(sc, dev, self.keep) if use_pre else None
        if use_pre:   # (the positional tensors are placeholders of the right shapes: fast_step does the same)
            xyz, rot, scaling, logit = self.keep[:4]
            self.args = (xyz, kw["shs"], e, logit, scaling, rot, e)
        else:
            self.args = (kw["means3D"], kw.get("shs", e), kw.get("colors_precomp", e), kw["opacities"], kw.get("scales", e), kw.get("rotations", e),
                         kw.get("cov3D_precomp", e))
        self.fw = rasterizer._forward_full(self.rs, *self.args, exact=True, pre=self.pre, invdepth=depth, antialiasing=aa)
        self.dL = sc.dL_dpix.to(dev)
        self.dD = _g_depth(sc)[None].to(dev) if depth else None

    def backward(self, focal=True, chain=None, fill=None):
        from das3r_amd import rasterizer
        I, _, _, geom, binning, img, cap = self.fw[:7]
        out = rasterizer._backward_impl(self.rs, I, self.dL, *self.args, geom, binning, img, cap, pre=self.pre, chain=chain,
                                        **({"grad_invdepth": self.dD} if self.dD is not None else {}),
                                        **({"focal": True, "focal_per_splat": True} if focal else {}), **({"_fill": fill} if fill is not None else {}))
        torch.cuda.synchronize()
        return [t.clone() if t is not None else None for t in out]


def _check_per_splat(what, per, ref, tol=None):
    """The bar of every per-Gaussian gradient; and a splat the oracle does not render contributes exactly nothing."""
    util.assert_grad_close(per.double().cpu().numpy(), ref.numpy(), f"{what} per-splat dL/d(log focal)", tol=tol, flips=True)


def _check_sums(what, sums, per):
    """sums against the float64 sum of the kernel's own per_splat: P 2^-24 sum |c_i| bounds the rounding of ANY order of P float32 additions
    (each of the P - 1 partial sums is at most sum |c_i| and is rounded once, to half an ulp: 2^-24 relative) — derived, not fitted."""
    P = per.shape[0]
    want, scale = per.double().sum(0), per.double().abs().sum(0)
    for axis in range(2):
        err, bar = abs(float(sums[axis].double() - want[axis])), P * 2.0 ** -24 * float(scale[axis])
        print(f"{what} axis {axis}: sums {float(sums[axis]):+.9e} per-splat total {float(want[axis]):+.9e} |delta| {err:.3e} bar {bar:.3e}")
        assert err <= bar, (what, axis, err, bar)


@pytest.mark.parametrize("name", VARIANTS)
def test_per_splat_against_the_oracles_per_splat_gradient(name):
    call = _Call(name)
    ref, scale = _reference(name)
    out = call.backward()
    sums, per = out[8], out[9]
    assert per.shape == (call.sc.P, 2) and torch.isfinite(per).all() and torch.isfinite(sums).all()
    _check_per_splat(name, per, ref)
    radii = call.fw[2]
    assert float(per[radii == 0].abs().max() if bool((radii == 0).any()) else 0.0) == 0.0, "a culled splat contributes exactly 0"
    _check_sums(name, sums, per)
    print(f"{name}: sums {sums.tolist()} oracle {ref.sum(0).tolist()} sum|c_i| {scale.tolist()}")


@pytest.mark.parametrize("name,depth,aa,use_pre", [("basic_deg3", True, False, False), ("long_lists", True, False, False),
                                                   ("aa_tiny", False, True, False), ("basic_deg3", False, True, False),
                                                   ("cov3D_precomp", False, True, False), ("aa_tiny", True, True, False),
                                                   ("basic_deg3", False, False, True), ("aa_tiny", True, True, True),
                                                   ("frustum_edge", True, True, False), ("aniso_focal", False, False, True),
                                                   ("portrait_world", True, False, False)])
def test_the_extra_modes_against_the_oracle(name, depth, aa, use_pre):
    """With dL_dinvdepth (the oracle image tests/test_gpu_invdepth.py uses), with antialiasing (the reference factor of
    tests/test_gpu_antialiasing.py), with in->pre (identity pose: the oracle's scene up to the rounding of log / exp and logit / sigmoid),
    and all three at once."""
    call = _Call(name, depth=depth, aa=aa, use_pre=use_pre)
    ref, _ = _reference(name, depth, aa)
    out = call.backward()
    _check_per_splat(f"{name} depth={depth} aa={aa} pre={use_pre}", out[9], ref)
    _check_sums(name, out[8], out[9])


def test_in_pre_with_a_pose_is_the_camera_frame_call_bit_for_bit(monkeypatch):
    """in->pre with a real pose: pretransform_math.h promises the bits of das3r_pretransform_forward, so the focal sums and every splat's share
    equal those of the call on the camera-frame tensors that kernel writes."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    from das3r_amd.fused import pretransform
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    _lib.reload_switches()
    try:
        sc, mode = _scene("basic_deg3")
        dev = _dev()
        keep = []
        _pre_of(sc, dev, keep)
        xyz, rot, scaling, logit, conf, _ = keep
        pose = torch.tensor([0.995, 0.05, -0.06, 0.04, 0.1, -0.05, 0.3], device=dev)
        with torch.no_grad():
            m3, r, s, o = pretransform(xyz, rot, scaling, logit, conf, None, pose)
        mats = torch.empty(28, device=dev)
        import ctypes as C
        _lib.check(_lib.load().das3r_pose_matrices(C.c_void_p(pose.data_ptr()), C.c_void_p(mats.data_ptr()), rasterizer._stream(dev)), "das3r_pose_matrices")
        pre = _lib.PreTransform()
        pre.xyz, pre.rot, pre.scaling, pre.opacity_raw = xyz.data_ptr(), rot.data_ptr(), scaling.data_ptr(), logit.data_ptr()
        pre.conf_flat, pre.mask_index = conf.data_ptr(), None
        pre.R, pre.t, pre.Lq = mats.data_ptr(), mats.data_ptr() + 36, mats.data_ptr() + 48
        rs = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()})
        e, shs, dL = torch.empty(0, device=dev), sc.shs.to(dev), sc.dL_dpix.to(dev)
        res = []
        for args, p in (((m3, shs, e, o, s, r, e), None), ((xyz, shs, e, logit, scaling, rot, e), pre)):
            fw = rasterizer._forward_full(rs, *args, exact=True, pre=p, antialiasing=True)
            out = rasterizer._backward_impl(rs, fw[0], dL, *args, fw[3], fw[4], fw[5], fw[6], pre=p, focal=True, focal_per_splat=True)
            torch.cuda.synchronize()
            res.append((fw[1], out[8], out[9]))
        assert torch.equal(res[0][0], res[1][0]), "the two forwards render the same bits"
        assert float(res[0][2].abs().max()) > 0
        assert torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][1], res[1][1])
    finally:
        monkeypatch.delenv("DAS3R_DETERMINISTIC")
        _lib.reload_switches()


# every backward compositing kernel the library can pick for these entries (forced as tests/test_gpu_antialiasing.py forces them); scan has
# no inverse-depth form (the entry refuses it there, as das3r_raster_backward_depth does)
BWD_ENVS = [
    (dict(DAS3R_RENDER_BWD="dpp"), True), (dict(DAS3R_RENDER_BWD="blk", DAS3R_BWD_BUCKETS="4"), True),
    (dict(DAS3R_RENDER="fine", DAS3R_RENDER_BWD="fine", DAS3R_BWD_BUCKETS="4"), True),
    (dict(DAS3R_RENDER_BWD="blk", DAS3R_BWD_BUCKETS="4", DAS3R_DETERMINISTIC="1"), True),
    (dict(DAS3R_RENDER_BWD="scan128"), False),
]


@pytest.mark.parametrize("env,with_depth", BWD_ENVS, ids=lambda e: "-".join(f"{k[6:]}={v}" for k, v in e.items()) if isinstance(e, dict) else str(e))
def test_focal_gradient_behind_every_backward_compositing_kernel(env, with_depth, monkeypatch):
    from das3r_amd import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _lib.reload_switches()
    try:
        tol = util.tolerances_for(env.get("DAS3R_RENDER_BWD"))["tol"]
        for depth in ((False, True) if with_depth else (False,)):
            call = _Call("long_lists", depth=depth, aa=True)   # (> 256 instances per tile: multi-batch, T < 1e-4 stops, the alpha clamp)
            ref, _ = _reference("long_lists", depth, True)
            out = call.backward()
            _check_per_splat(f"{env} depth={depth}", out[9], ref, tol=tol)
            _check_sums(str(env), out[8], out[9])
        if not with_depth:
            with pytest.raises(RuntimeError, match="das3r_raster_backward_focal: DAS3R_RENDER_BWD=scan has no inverse-depth form"):
                _Call("single", depth=True).backward()
    finally:
        for k in env:
            monkeypatch.delenv(k)
        _lib.reload_switches()


def test_both_row_forms(monkeypatch):
    """The rows of a splat come in two forms (launch_render_backward's quad_rows): nine sums per instance — every kernel above — and the stream
    kernel's up to four rows of twelve per instance, which only a library built with EXPERIMENTS=1 carries.  There the focal kernel folds
    that form too; the shipped library refuses the forced kernel before anything is launched."""
    from das3r_amd import _lib
    monkeypatch.setenv("DAS3R_RENDER_BWD", "stream")
    _lib.reload_switches()
    try:
        if _lib.has_experiments():
            call = _Call("long_lists")
            ref, _ = _reference("long_lists")
            out = call.backward()
            _check_per_splat("stream rows", out[9], ref, tol=util.GRAD_REL_TOL_SPLIT)
            _check_sums("stream rows", out[8], out[9])
        else:
            with pytest.raises(RuntimeError, match="built without the superseded kernels"):
                _Call("single").backward()
    finally:
        monkeypatch.delenv("DAS3R_RENDER_BWD")
        _lib.reload_switches()


@pytest.mark.parametrize("depth", [False, True])
def test_deterministic_prefilled_and_no_effect_on_the_other_gradients(depth, monkeypatch):
    """With the compositing backward in its fixed-order form (DAS3R_DETERMINISTIC=1: the pixel-per-lane kernel meets its waves in LDS float
    atomics, so the ROWS the focal kernel reads vary from run to run otherwise) two calls give the same bits; sums, per_splat, the workspace
    and the whole scratch filled with NaN beforehand change nothing; and the gradient tensors of das3r_raster_backward_focal are those of
    das3r_raster_backward / _depth bit for bit."""
    from das3r_amd import _lib
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    _lib.reload_switches()
    try:
        for name in ("basic_deg3", "culled"):
            call = _Call(name, depth=depth, aa=name == "culled")
            a, b = call.backward(), call.backward()
            assert float(a[9].abs().max()) > 0
            assert torch.equal(a[8], b[8]) and torch.equal(a[9], b[9]), "two runs differ"
            c = call.backward(fill=float("nan"))
            assert torch.equal(a[8], c[8]) and torch.equal(a[9], c[9]), "a pre-filled output or workspace reaches the result"
            plain = call.backward(focal=False)
            for k, (x, y) in enumerate(zip(a[:8], plain)):
                assert (x is None) == (y is None), GRAD_NAMES[k]
                assert x is None or torch.equal(x, y), f"dL/d{GRAD_NAMES[k]} differs between the focal entry and the plain one"
                assert x is None or c[k] is None or torch.equal(x, c[k])
    finally:
        monkeypatch.delenv("DAS3R_DETERMINISTIC")
        _lib.reload_switches()


def test_nothing_rendered_and_no_splats():
    """P == 0 or nothing rendered: sums = 0 and per_splat = 0, whatever the buffers held."""
    from das3r_amd import GaussianRasterizationSettings, rasterizer
    dev = _dev()
    sc, mode = _scene("deg0")
    sc.means3D[:, 2] = -1.0   # everything behind the camera
    rs = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()})
    e = torch.empty(0, device=dev)
    for P in (sc.P, 0):
        args = (sc.means3D[:P].to(dev), sc.shs[:P].to(dev), e, sc.opacities[:P].to(dev), sc.scales[:P].to(dev), sc.rotations[:P].to(dev), e)
        fw = rasterizer._forward_full(rs, *args, exact=True)
        assert fw[0] == 0
        out = rasterizer._backward_impl(rs, fw[0], sc.dL_dpix.to(dev), *args, fw[3], fw[4], fw[5], fw[6], focal=True, focal_per_splat=True,
                                        **({"_fill": float("nan")} if P else {}))
        torch.cuda.synchronize()
        assert out[8].shape == (2,) and float(out[8].abs().max()) == 0.0
        assert out[9].shape == (P, 2) and (P == 0 or float(out[9].abs().max()) == 0.0)


def test_chained_form(monkeypatch):
    """grads->chain (the Adam step of the raw parameters inside the per-Gaussian backward): the focal kernel runs before that step, so its sums
    are those of the unchained call on equal inputs, bit for bit, and the updated parameters and moments are those of a chained
    das3r_raster_backward."""
    from das3r_amd import _lib
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    _lib.reload_switches()
    try:
        call = _Call("culled", use_pre=True, sh_cols=4, aa=True)   # (degree 1, M = 4: an unstaged SH layout, which the chain needs)
        xyz, rot, scaling, logit, conf, _ = call.keep
        params = [xyz, rot, scaling, logit]
        start = [p.clone() for p in params]
        unchained = call.backward()

        def step(focal):
            for p, p0 in zip(params, start):
                p.copy_(p0)
            m, v = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
            slots = (_lib.AdamSlot * 4)()
            for k in range(4):
                slots[k].param, slots[k].exp_avg, slots[k].exp_avg_sq = params[k].data_ptr(), m[k].data_ptr(), v[k].data_ptr()
                slots[k].step_size, slots[k].bc2_sqrt = 1e-3, math.sqrt(1.0 - 0.999)
            g_conf, g_small = torch.zeros_like(conf), torch.zeros(28, device=call.dev)
            chain = _lib.Chain()
            chain.g_conf_flat, chain.g_small, chain.slots = g_conf.data_ptr(), g_small.data_ptr(), slots
            chain.beta1, chain.beta2, chain.eps = 0.9, 0.999, 1e-15
            out = call.backward(focal=focal, chain=chain)
            return out, [t.clone() for t in params + m + v] + [g_conf.clone(), g_small.clone()]

        with_focal, state_f = step(True)
        _, state_p = step(False)
        for p, p0 in zip(params, start):
            p.copy_(p0)
        assert not torch.equal(state_f[0], start[0]), "a step was taken"
        assert torch.equal(with_focal[8], unchained[8]) and torch.equal(with_focal[9], unchained[9])
        for k, (a, b) in enumerate(zip(state_f, state_p)):
            assert torch.equal(a, b), k
    finally:
        monkeypatch.delenv("DAS3R_DETERMINISTIC")
        _lib.reload_switches()


@pytest.mark.parametrize("invdepth,aa", [(False, False), (True, False), (False, True), (True, True)])
def test_autograd_log_focal_through_the_drop_in_rasterizer(invdepth, aa):
    """GaussianRasterizer(...)(..., log_focal=...): FoVx.grad / FoVy.grad of s = -log tan(FoV / 2) against the oracle's sum chained through
    -1 / sin(FoV), at the per-Gaussian bar relative to sum |c_i| / sin(FoV); every other gradient is the call's without log_focal."""
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer
    from das3r_amd.model import log_focal_of
    name = "aa_tiny" if aa else "basic_deg3"
    sc, mode = _scene(name)
    dev = _dev()
    ref, scale = _reference(name, invdepth, aa)
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()}
    fov = [torch.tensor(2 * math.atan(t), device=dev, requires_grad=True) for t in (sc.tanfovx, sc.tanfovy)]
    gD = _g_depth(sc).to(dev)

    def run(log_focal):
        kw = {k: v.to(dev).clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
        m2d = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
        res = GaussianRasterizer(GaussianRasterizationSettings(**skw))(means2D=m2d, **kw, return_invdepth=invdepth, antialiasing=aa,
                                                                         **({"log_focal": log_focal} if log_focal is not None else {}))
        loss = (res[0] * sc.dL_dpix.to(dev)).sum() + ((res[2][0] * gD).sum() if invdepth else 0.0)
        loss.backward()
        return res[0].detach(), {**{k: v.grad for k, v in kw.items()}, "means2D": m2d.grad}

    img, g = run(log_focal_of(fov[0], fov[1]))
    img0, g0 = run(None)
    assert torch.equal(img, img0)
    for k in g0:
        assert torch.allclose(g[k], g0[k], rtol=0, atol=util.GRAD_REL_TOL * float(g0[k].abs().max())), k   # (the dpp kernel's rows vary run to run)
    for axis in range(2):
        sin = math.sin(float(fov[axis].detach()))
        want = -float(ref[:, axis].sum()) / sin
        bar = util.GRAD_REL_TOL * float(scale[axis]) / sin
        print(f"{name} invdepth={invdepth} aa={aa} axis {axis}: FoV.grad {float(fov[axis].grad):+.8e} oracle {want:+.8e} bar {bar:.3e}")
        assert abs(float(fov[axis].grad) - want) <= bar, (axis, float(fov[axis].grad), want, bar)
    # a log_focal that takes no gradient: today's backward, no focal call
    run(log_focal_of(fov[0].detach(), fov[1].detach()))


def _small_model(seed=3, fov_lr=0.0, fused=False, focal_scale=1.0, psnr_threshold=None, **seq_kw):
    import copy
    from das3r_amd.camera import focal2fov
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    seq_kw = seq_kw or dict(frames=3, W=32, H=24, focal=0.9 * 32, n_splats=1500)
    seq = synthetic_sequence(seed=seed, **seq_kw)
    model, cams = build_from_sequence(copy.deepcopy(seq))
    if focal_scale != 1.0:
        model.init_fov(focal2fov(seq["focal"] * focal_scale, seq["W"]), focal2fov(seq["focal"] * focal_scale, seq["H"]))
    opt = OptimParams(iterations=100, **({"fov_lr": fov_lr} if fov_lr else {}), **({"psnr_threshold": psnr_threshold} if psnr_threshold is not None else {}))
    model.training_setup(opt, fused=fused)
    return model, cams, opt, seq


def test_das3r_render_sends_the_gradient_to_the_models_field_of_view():
    """das3r_render at fov_lr > 0 renders with the model's field of view (here 2 % off the camera's) and autograd reaches FoVx / FoVy: against
    the oracle on the very tensors the rasterizer was handed, chained through -1 / sin, at the per-Gaussian bar relative to sum |c_i| / sin."""
    from das3r_amd.render import das3r_render, rasterizer_inputs
    model, cams, opt, _ = _small_model(fov_lr=1e-3, focal_scale=1.02)
    dev = _dev()
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    cam, uid = cams[1], 1
    g_pix = torch.randn(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(8)).to(dev)
    pkg = das3r_render(cam, model, PIPE, bg, camera_pose=model.get_RT(uid))
    (pkg["render"] * g_pix).sum().backward()
    assert model.FoVx.grad is not None and model.FoVy.grad is not None
    with torch.no_grad():
        settings, kw = rasterizer_inputs(cam, model, PIPE, bg, camera_pose=model.get_RT(uid))
    assert "log_focal" in kw and settings.tanfovx == pytest.approx(math.tan(0.5 * float(model.FoVx)), rel=1e-6)
    assert abs(settings.tanfovx / math.tan(0.5 * cam.FoVx) - 1 / 1.02) < 1e-3, "the settings come from the model's field of view"
    okw = {k: kw[k].detach().double() for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    skw = {k: v for k, v in settings._asdict().items() if k not in ("prefiltered", "debug")}
    c, _ = fr.per_splat_from(okw, skw, g_pix.double())
    for axis, t in enumerate((model.FoVx, model.FoVy)):
        sin = math.sin(float(t))
        want, bar = -float(c[:, axis].sum()) / sin, util.GRAD_REL_TOL * float(c[:, axis].abs().sum()) / sin
        print(f"das3r_render axis {axis}: FoV.grad {float(t.grad):+.8e} oracle {want:+.8e} bar {bar:.3e}")
        assert abs(float(t.grad) - want) <= bar, (axis, float(t.grad), want, bar)


@pytest.mark.parametrize("fused", [False, True])
def test_fov_lr_zero_never_calls_the_focal_entry(fused, monkeypatch):
    """At the default fov_lr = 0 three train steps, autograd and direct, never reach das3r_raster_backward_focal, render with the camera's
    field of view and leave FoVx / FoVy as they were."""
    from das3r_amd import _lib, fast_step
    from das3r_amd.train import train_step

    def refuse(*a, **k):
        raise AssertionError("das3r_raster_backward_focal called at fov_lr = 0")
    monkeypatch.setattr(_lib.load(), "das3r_raster_backward_focal", refuse)
    model, cams, opt, _ = _small_model(fused=fused, psnr_threshold=0.0)
    assert fast_step.available(model, PIPE) == fused and model.fov_lr == 0.0
    assert [g["name"] for g in model.optimizer_cam.param_groups] == (["pose_Q", "pose_T"] if fused else ["pose_Q", "pose_T", "fovX", "fovY"])
    assert fused or [g["lr"] for g in model.optimizer_cam.param_groups[2:]] == [0.0001, 0.0001]
    before = (model.FoVx.detach().clone(), model.FoVy.detach().clone(), model.Q.detach().clone())
    bg = torch.zeros(3, device=_dev())
    for it, u in enumerate([0, 2, 1], start=1):
        train_step(model, cams[u], opt, it, PIPE, bg, fused=fused)
    torch.cuda.synchronize()
    assert torch.equal(model.FoVx.detach(), before[0]) and torch.equal(model.FoVy.detach(), before[1]) and model.FoVx.grad is None
    assert not torch.equal(model.Q.detach(), before[2]), "the camera optimizer did step"
    with pytest.raises(AssertionError, match="called at fov_lr = 0"):   # (the wrapper is in the path a focal backward takes)
        model.fov_lr = 1e-3
        train_step(model, cams[0], opt, 4, PIPE, bg, fused=fused)


def test_direct_and_autograd_steps_agree_on_the_field_of_view():
    """Three steps with fov_lr > 0 (gate open: psnr_threshold 0), the direct fused step against the autograd fused step: FoVx / FoVy agree at
    the bar tests/test_gpu_trainstep.py holds the pose rows to (|a - b| <= 1e-5 + 1e-4 |b| on all but 1e-3 of the elements — of two: on both),
    and so do the poses."""
    from das3r_amd import fast_step
    from das3r_amd.train import train_step
    out = []
    for direct in (True, False):
        model, cams, opt, _ = _small_model(seed=9, fov_lr=1e-3, fused=True, focal_scale=1.03, psnr_threshold=0.0)
        model.fast_step = direct
        assert fast_step.available(model, PIPE) == direct
        assert [g["name"] for g in model.optimizer_cam.param_groups] == ["pose_Q", "pose_T", "fovX", "fovY"]
        assert [g["lr"] for g in model.optimizer_cam.param_groups[2:]] == [1e-3, 1e-3]
        start = torch.stack((model.FoVx.detach(), model.FoVy.detach())).clone()
        bg = torch.zeros(3, device=_dev())
        losses = [float(train_step(model, cams[u], opt, it, PIPE, bg, fused=True)[0]) for it, u in enumerate([0, 2, 1], start=1)]
        out.append((losses, start, torch.stack((model.FoVx.detach(), model.FoVy.detach())).clone(), model.Q.detach().clone(), model.T.detach().clone()))
    (la, s_a, fa, qa, ta), (lb, s_b, fb, qb, tb) = out
    assert torch.equal(s_a, s_b) and not torch.equal(fa, s_a), "the field of view moved"
    print("FoV direct", fa.tolist(), "autograd", fb.tolist(), "start", s_a.tolist())
    print("losses direct", la, "autograd", lb)
    for a, b in ((fa, fb), (qa, qb), (ta, tb)):
        far = (a - b).abs() > 1e-5 + 1e-4 * b.abs()
        assert float(far.double().mean()) <= 1e-3, (a, b)


TRAIN_ITERATIONS = 40   # (Adam moves FoV by about fov_lr = 1e-3 rad a step; 3 % of focal is 0.026 rad at this field of view)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_training_pulls_a_wrong_focal_length_back(seed):
    """train.synthetic_sequence at its default small shape; the model's focal length starts 3 % above the sequence's.  With fov_lr > 0 the
    error |log(f_model / f_true)| after TRAIN_ITERATIONS direct fused steps is below its start, in x and in y; with fov_lr = 0 the field of
    view is unchanged bit for bit.  Q / T train as always (at 3e-5 a step they cannot absorb the error in forty steps: a 3 % zoom is
    0.15 units of camera z at this depth).  The gate is open (psnr_threshold 0): a 3 % zoom error alone keeps a frame below 26 dB."""
    from das3r_amd.train import train
    err = {}
    for fov_lr in (1e-3, 0.0):
        model, cams, opt, seq = _small_model(seed=seed, fov_lr=fov_lr, fused=True, focal_scale=1.03, psnr_threshold=0.0, frames=6)
        f_true = (seq["W"] / (2 * math.tan(0.5 * cams[0].FoVx)), seq["H"] / (2 * math.tan(0.5 * cams[0].FoVy)))
        focal = lambda: (seq["W"] / (2 * math.tan(0.5 * float(model.FoVx))), seq["H"] / (2 * math.tan(0.5 * float(model.FoVy))))
        e0 = [abs(math.log(f / t)) for f, t in zip(focal(), f_true)]
        before = (model.FoVx.detach().clone(), model.FoVy.detach().clone())
        train(model, cams, opt, TRAIN_ITERATIONS, pipe=PIPE, seed=seed, fused=True)
        e1 = [abs(math.log(f / t)) for f, t in zip(focal(), f_true)]
        err[fov_lr] = (e0, e1)
        print(f"seed {seed} fov_lr {fov_lr:g}: |log(f_model / f_true)| start {e0[0]:.5f} / {e0[1]:.5f} -> end {e1[0]:.5f} / {e1[1]:.5f}")
        if fov_lr == 0.0:
            assert torch.equal(model.FoVx.detach(), before[0]) and torch.equal(model.FoVy.detach(), before[1])
        else:
            assert abs(e0[0] - math.log(1.03)) < 1e-4 and e1[0] < e0[0] and e1[1] < e0[1], (seed, e0, e1)
