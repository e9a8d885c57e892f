"""GPU tests of the antialiasing mode (das3r_raster_saved.flags bit 4, upstream's 2D mip filter): every splat is blended with its
opacity times f = sqrt(max(rho, 2.5e-5)), rho = det(T Sigma T^T) / det(T Sigma T^T + 0.3 I), and the backward differentiates f.

The reference is the float64 dense oracle fed opacities * f, with f taken from the conic of a first dense call (the same autograd
graph, so one reference gives the image and the exact gradients)."""
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

RHO_MIN = 2.5e-5
GRAD_KEYS = ("means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _scene(name):
    """util.scene_variant, plus "aa_tiny": splats from well below a pixel to a few pixels, half of them at opacity 0.99 — the smallest ones sit
    at the 2.5e-5 clamp of rho and are still blended (0.99 sqrt(2.5e-5) > 1/255)."""
    if name != "aa_tiny":
        return util.scene_variant(name)
    from das3r_amd.synth import make_scene
    sc = make_scene(P=1500, W=96, H=64, focal=80.0, sh_degree=2, seed=41, s_px=(0.01, 4.0), bg=(0.1, 0.2, 0.3))
    sc.opacities[: sc.P // 2] = 0.99
    return sc, dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)


def aa_factor(conic):
    """f of the dense oracle's conic (A, B, C) = (c, -b, a) / det: the un-dilated entries are a - 0.3 and c - 0.3."""
    A, B, C = conic[:, 0], conic[:, 1], conic[:, 2]
    det = 1.0 / (A * C - B * B)
    a, b, c = C * det, -B * det, A * det
    rho = ((a - 0.3) * (c - 0.3) - b * b) / det
    return torch.sqrt(torch.clamp(rho, min=RHO_MIN)), rho


def _oracle(sc, mode, dev, gD=None):
    """(color, {input: dL/dinput}, rho) of <dL_dpix, color> (+ <gD, invdepth>) for the antialiased forward, float64 autograd."""
    from oracle.dense_oracle import rasterize_dense
    kw = {k: v.to(dev).double().clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items() if k not in ("prefiltered", "debug")}
    m2d = torch.zeros(sc.P, 3, dtype=torch.float64, device=dev, requires_grad=True)
    _, _, aux = rasterize_dense(means2D=m2d, **kw, **skw)
    f, rho = aa_factor(aux["conic"])
    kw_aa = dict(kw, opacities=kw["opacities"] * f[:, None])
    color, _, _ = rasterize_dense(means2D=m2d, **kw_aa, **skw)
    loss = (color * sc.dL_dpix.to(dev).double()).sum()
    if gD is not None:
        V = torch.as_tensor(skw["viewmatrix"]).double().reshape(4, 4)
        m = kw["means3D"]
        z = (torch.cat([m, torch.ones(m.shape[0], 1, dtype=torch.float64, device=dev)], 1) @ V[:, 2:3]).reshape(-1)
        inv = (1.0 / z.clamp_min(1e-6))[:, None].expand(-1, 3)
        dkw = {k: v for k, v in kw_aa.items() if k not in ("shs", "colors_precomp")}
        depth, _, _ = rasterize_dense(means2D=m2d, colors_precomp=inv, **dkw, **dict(skw, bg=torch.zeros(3, dtype=torch.float64, device=dev)))
        loss = loss + (depth[0] * gD.to(dev).double()).sum()
    loss.backward()
    g = {k: v.grad for k, v in kw.items()}
    g["means2D"] = m2d.grad
    return color.detach(), g, rho.detach()


def _hip(sc, mode, dev, aa, gD=None):
    """(color, radii, grads) through the drop-in rasterizer."""
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer
    kw = {k: v.to(dev).clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()}
    m2d = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    res = GaussianRasterizer(GaussianRasterizationSettings(**skw))(means2D=m2d, **kw, antialiasing=aa, return_invdepth=gD is not None)
    loss = (res[0] * sc.dL_dpix.to(dev)).sum() + ((res[2][0] * gD.to(dev)).sum() if gD is not None else 0.0)
    loss.backward()
    g = {k: v.grad for k, v in kw.items()}
    g["means2D"] = m2d.grad
    return res[0].detach(), res[1], g


def _num_rendered(sc, mode, dev, aa):
    from das3r_amd import GaussianRasterizationSettings, rasterizer
    kw = {k: v.to(dev) for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()}
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(GaussianRasterizationSettings(**skw), kw["means3D"], kw.get("shs", e), kw.get("colors_precomp", e), kw["opacities"],
                                   kw.get("scales", e), kw.get("rotations", e), kw.get("cov3D_precomp", e), exact=True, antialiasing=aa)
    return res[0], res[2]


def _check(name, color, g, ref_color, ref_g, tol=None, scale_modifier=1.0):
    util.assert_color_close(color.double().cpu().numpy(), ref_color.cpu().numpy(), f"{name} antialiased colour")
    for k in GRAD_KEYS:
        if k in ref_g:
            ref = ref_g[k] / scale_modifier if k == "scales" else ref_g[k]   # (upstream's dL/dscale is dL/d(scale_modifier * scale))
            util.assert_grad_close(g[k].double().cpu().numpy(), ref.cpu().numpy(), f"{name} antialiased dL/d{k}", tol=tol)


# ("deep", ~4000 faint layers per tile, is left out: with the factor one of its pixels meets T < 1e-4 one splat later in fp32 than in fp64 —
#  a threshold flip of 3e-3 of the gradient maxima on the splats of that pixel, everything else within the bars)
@pytest.mark.parametrize("name", ["aa_tiny", "basic_deg3", "long_lists", "ragged_image", "culled", "deg0", "colors_precomp", "cov3D_precomp",
                                  "scale_modifier", "world_camera"] + util.CAMERA_VARIANTS)
def test_antialiased_forward_and_backward_against_the_dense_oracle(name):
    sc, mode = _scene(name)
    dev = _dev()
    ref_color, ref_g, rho = _oracle(sc, mode, dev)
    color, radii, g = _hip(sc, mode, dev, True)
    _check(name, color, g, ref_color, ref_g, scale_modifier=mode["scale_modifier"])
    _, radii0, _ = _hip(sc, mode, dev, False)
    assert torch.equal(radii, radii0), "radii do not depend on the mode"
    n_aa, _ = _num_rendered(sc, mode, dev, True)
    n0, _ = _num_rendered(sc, mode, dev, False)
    assert n_aa <= n0, (n_aa, n0)   # (the opacity-aware tile box shrinks with the opacity)
    if name == "aa_tiny":   # the clamped branch is exercised by splats that are blended
        vis = (radii > 0).cpu()
        clamped = vis & (rho.cpu() < RHO_MIN) & (sc.opacities[:, 0] > 0.9)
        assert int(clamped.sum()) >= 10, int(clamped.sum())
        ref_plain, _, _ = _oracle_plain(sc, mode, dev)
        assert float((ref_plain - ref_color).abs().max()) > 1e-2   # (the mode changes the image)


def _oracle_plain(sc, mode, dev):
    from oracle.dense_oracle import rasterize_dense
    kw = {k: v.to(dev).double() for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items() if k not in ("prefiltered", "debug")}
    return rasterize_dense(means2D=torch.zeros(sc.P, 3, dtype=torch.float64, device=dev), **kw, **skw)


KERNEL_ENVS = [
    dict(DAS3R_RENDER="quad"), dict(DAS3R_RENDER="rows"), dict(DAS3R_RENDER="lanes"), dict(DAS3R_RENDER="slices"),
    dict(DAS3R_RENDER="quad", DAS3R_BINNING="local"), dict(DAS3R_RENDER="rows", DAS3R_BINNING="seg"),
    dict(DAS3R_RENDER_BWD="dpp"), dict(DAS3R_RENDER_BWD="blk", DAS3R_BWD_BUCKETS="4"),
    dict(DAS3R_RENDER="fine", DAS3R_RENDER_BWD="fine", DAS3R_BWD_BUCKETS="4"),
    dict(DAS3R_RENDER_BWD="blk", DAS3R_BWD_BUCKETS="4", DAS3R_DETERMINISTIC="1"),
    dict(DAS3R_RENDER_BWD="scan128"),
]


@pytest.mark.parametrize("env", KERNEL_ENVS, ids=lambda e: "-".join(f"{k[6:]}={v}" for k, v in e.items()))
def test_antialiasing_through_every_compositing_kernel(env, monkeypatch):
    """Bit 4 travels with the region / hint bits of flags: each forced forward and backward kernel gives the antialiased image and gradients."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, mode = util.scene_variant("long_lists")   # (> 256 instances per tile: multi-batch, T < 1e-4 stops, the alpha clamp)
    dev = _dev()
    ref_color, ref_g, _ = _oracle(sc, mode, dev)
    color, _, g = _hip(sc, mode, dev, True)
    _check(str(env), color, g, ref_color, ref_g, tol=util.tolerances_for(env.get("DAS3R_RENDER_BWD"))["tol"])


@pytest.mark.parametrize("bwd,name", [pytest.param(b, n, id=b if n == "aa_tiny" else f"{b}-{n}") for n in ("aa_tiny", "portrait_world")
                                      for b in ("dpp", "blk", "fine")])
def test_antialiased_backward_depth_against_the_dense_oracle(bwd, name, monkeypatch):
    """das3r_raster_backward_depth with bit 4: the factor's derivative is applied once, to the opacity sums of both passes."""
    monkeypatch.setenv("DAS3R_RENDER_BWD", bwd)
    if bwd == "fine":
        monkeypatch.setenv("DAS3R_RENDER", "fine")
    if bwd != "dpp":
        monkeypatch.setenv("DAS3R_BWD_BUCKETS", "4")
    sc, mode = _scene(name)
    dev = _dev()
    gD = torch.randn(sc.H, sc.W, generator=torch.Generator().manual_seed(5)) * 0.5
    _, ref_g, _ = _oracle(sc, mode, dev, gD)
    _, _, g = _hip(sc, mode, dev, True, gD)
    for k in ref_g:
        util.assert_grad_close(g[k].double().cpu().numpy(), ref_g[k].cpu().numpy(), f"{name} {bwd} depth dL/d{k}")


def _direct(sc, mode, dev, invdepth, flags_mask=~0):
    """_forward_full + _backward_impl with antialiasing; flags_mask clears bits of the flags handed back."""
    from das3r_amd import GaussianRasterizationSettings, rasterizer
    kw = {k: v.to(dev) for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()}
    rs = GaussianRasterizationSettings(**skw)
    e = torch.empty(0, device=dev)
    args = (kw["means3D"], kw.get("shs", e), kw.get("colors_precomp", e), kw["opacities"], kw.get("scales", e), kw.get("rotations", e),
            kw.get("cov3D_precomp", e))
    res = rasterizer._forward_full(rs, args[0], args[1], args[2], args[3], args[4], args[5], args[6], invdepth=invdepth, antialiasing=True)
    cap = res[6]
    cap.flags = cap.flags & flags_mask
    gD = (torch.randn(1, sc.H, sc.W, generator=torch.Generator().manual_seed(5)) * 0.5).to(dev) if invdepth else None
    g = rasterizer._backward_impl(rs, res[0], sc.dL_dpix.to(dev), args[0], args[1], args[2], args[3], args[4], args[5], args[6],
                                  res[3], res[4], res[5], cap, grad_invdepth=gD)
    return res, g, gD


@pytest.mark.parametrize("invdepth", [False, True])
def test_drop_in_rasterizer_equals_the_direct_calls_bit_for_bit(invdepth, monkeypatch):
    from das3r_amd import _lib
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    sc, mode = _scene("aa_tiny")
    dev = _dev()
    res, gd, gD = _direct(sc, mode, dev, invdepth)
    assert res[6].flags & _lib.ANTIALIAS_FLAG
    g_m2d, _, g_op, g_m3d, _, g_sh, g_sc, g_rot = gd
    color, _, g = _hip(sc, mode, dev, True, gD[0].cpu() if invdepth else None)
    assert torch.equal(color, res[1])
    for k, want in (("means2D", g_m2d), ("opacities", g_op), ("means3D", g_m3d), ("shs", g_sh), ("scales", g_sc), ("rotations", g_rot)):
        assert torch.equal(g[k], want.reshape(g[k].shape)), k


@pytest.mark.parametrize("name", ["basic_deg3", "cov3D_precomp"])
def test_jacobian_and_row_backward_agree_bit_for_bit_with_antialiasing(name, monkeypatch):
    """The JAC form (flags bit 2 handed back) and the SH-row form (bit 2 cleared, bit 4 kept) give the same antialiased gradients bit for bit."""
    from das3r_amd import _lib
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    sc, mode = util.scene_variant(name)
    dev = _dev()
    res_a, ga, _ = _direct(sc, mode, dev, False)
    assert res_a[6].flags & 4 and res_a[6].flags & _lib.ANTIALIAS_FLAG
    res_b, gb, _ = _direct(sc, mode, dev, False, flags_mask=~4)
    assert torch.equal(res_a[1], res_b[1])
    for x, y in zip(ga, gb):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("degree", [0, 1, 3])
def test_direct_fused_step_with_antialiasing_matches_the_autograd_fused_step(degree):
    """pipe.antialiasing = True in the direct iteration (fast_step: the chained DEG0 / degree-1 forms, the pre-transform + JAC form at degree 3,
    and the two-kernel "grads" form) against the autograd iteration through das3r_render(fused=True), over four steps, at the bars of
    test_gpu_trainstep.py::test_direct_fused_step_matches_the_autograd_fused_step."""
    from types import SimpleNamespace
    from das3r_amd import fast_step
    from das3r_amd.train import train_step
    from tests.test_gpu_trainstep import NAMES, _pair
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False, antialiasing=True)
    out = []
    for direct in (True, False, "grads"):
        model, cams, _, opt, _dense = _pair(frames=3, W=32, H=24, seed=9, heldout=False, iterations=100, fused=True, generic=True)
        model.fast_step = bool(direct)
        model.fuse_geometry_adam = direct is True
        assert fast_step.available(model, pipe) == bool(direct)
        model.active_sh_degree = degree
        model.optimizer.set_active_sh_degree(degree)
        with torch.no_grad():
            g = torch.Generator(device="cpu").manual_seed(11)
            model._features_rest.copy_((torch.randn(model._features_rest.shape, generator=g) * 0.05).to(model._features_rest.device))
        bg = torch.zeros(3, device="cuda")
        rec = []
        for it, u in enumerate([0, 2, 1, 0], start=1):
            loss, ps, pkg = train_step(model, cams[u], opt, it, pipe, bg, fused=True)
            rec.append((float(loss), float(ps), pkg["viewspace_points"].grad.detach().clone(), int(pkg["visibility_filter"].sum())))
        st = model.optimizer.state[model._features_rest]
        out.append((rec, {k: getattr(model, a).detach().clone() for k, a in NAMES.items()}, st["exp_avg"].clone(), st["step"],
                    model.optimizer_cam._gate_state.clone()))
    ref = out[1]
    for form in (out[0], out[2]):
        (ra, pa, ma, sa, ga), (rb, pb, mb, sb, gb) = form, ref
        assert sa == sb == 4 and torch.equal(ga, gb)
        for (la, psa, m2a, va), (lb, psb, m2b, vb) in zip(ra, rb):
            assert abs(la - lb) <= 1e-6 * abs(lb) and abs(psa - psb) <= 1e-4 and va == vb, (la, lb, psa, psb)
            assert torch.allclose(m2a, m2b, rtol=1e-4, atol=1e-7 * float(m2b.abs().max()))
        assert torch.allclose(ma, mb, rtol=1e-4, atol=1e-9)
        for k in pa:
            far = (pa[k] - pb[k]).abs() > 1e-5 + 1e-4 * pb[k].abs()
            assert float(far.double().mean()) <= 1e-3, (k, float(far.double().mean()))
    # and the mode is on: the same first step without it renders another loss
    model, cams, _, opt, _dense = _pair(frames=3, W=32, H=24, seed=9, heldout=False, iterations=100, fused=True, generic=True)
    model.active_sh_degree = degree
    model.optimizer.set_active_sh_degree(degree)
    with torch.no_grad():
        g = torch.Generator(device="cpu").manual_seed(11)
        model._features_rest.copy_((torch.randn(model._features_rest.shape, generator=g) * 0.05).to(model._features_rest.device))
    plain = float(train_step(model, cams[0], opt, 1, SimpleNamespace(**{**vars(pipe), "antialiasing": False}), torch.zeros(3, device="cuda"), fused=True)[0])
    assert plain != out[0][0][0][0]


def _mass_field(W, H, focal, seed=3, P=256, focal_full=400.0):
    """Non-overlapping, low-opacity splats of 0.3 - 2 px at full resolution (focal_full) on a grid, colour 1, background 0."""
    from das3r_amd.synth import Scene
    from das3r_amd.camera import projection_matrix
    import math
    g = torch.Generator().manual_seed(seed)
    n = int(math.isqrt(P))
    tanfovx, tanfovy = W / (2.0 * focal), H / (2.0 * focal)
    z = 5.0
    u = (torch.arange(n) + 0.5) / n * 1.8 - 0.9
    uu, vv = torch.meshgrid(u, u, indexing="xy")
    x, y = uu.reshape(-1) * z * tanfovx, vv.reshape(-1) * z * tanfovy
    Pn = x.numel()
    means3D = torch.stack([x, y, torch.full_like(x, z)], 1).contiguous()
    spx = torch.exp(torch.rand(Pn, generator=g) * math.log(2.0 / 0.3)) * 0.3
    scales = (spx[:, None].expand(-1, 3) * z / focal_full).contiguous()   # (world units: the same field at both resolutions)
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]]).expand(Pn, -1).contiguous()
    fovx, fovy = 2 * math.atan(tanfovx), 2 * math.atan(tanfovy)
    proj = (torch.eye(4) @ projection_matrix(0.01, 100.0, fovx, fovy).transpose(0, 1)).contiguous()
    return Scene(W=W, H=H, tanfovx=tanfovx, tanfovy=tanfovy, sh_degree=0, viewmatrix=torch.eye(4), projmatrix=proj, campos=torch.zeros(3),
                 bg=torch.zeros(3), means3D=means3D, scales=scales, rotations=rot, opacities=torch.full((Pn, 1), 0.2),
                 shs=torch.zeros(Pn, 1, 3), dL_dpix=torch.zeros(3, H, W))


def test_antialiasing_keeps_the_image_mass_across_resolutions():
    """The mode does what it is for: a field of small, separate, faint splats rendered at W x H and at W/2 x H/2 (same field of view) keeps
    its image mass (sum over pixels in full-resolution pixel areas, colour 1, background 0) closer with antialiasing.  Without it the half-resolution image gains mass —
    the fixed 0.3 px^2 dilation is a larger share of every splat; with it the factor takes that back.  Bar: the relative change with the
    mode is below half the change without it — loose on purpose (a deterministic render; the assertion message gives both changes)."""
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer
    dev = _dev()
    mass = {}
    for aa in (False, True):
        for W, H, focal in ((256, 256, 400.0), (128, 128, 200.0)):
            sc = _mass_field(W, H, focal)
            skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.settings_kwargs().items()}
            with torch.no_grad():
                img, _ = GaussianRasterizer(GaussianRasterizationSettings(**skw))(
                    means3D=sc.means3D.to(dev), means2D=torch.zeros(sc.P, 3, device=dev), opacities=sc.opacities.to(dev),
                    colors_precomp=torch.ones(sc.P, 3, device=dev), scales=sc.scales.to(dev), rotations=sc.rotations.to(dev), antialiasing=aa)
            mass[(aa, W)] = float(img[0].double().sum()) * (256 // W) ** 2   # (in full-resolution pixel areas)
    change = {aa: abs(mass[(aa, 128)] - mass[(aa, 256)]) / mass[(aa, 256)] for aa in (False, True)}
    assert change[True] < 0.5 * change[False], (change, mass)
