"""GPU tests of the inverse-depth output (ABI 16, das3r_raster_out.out_invdepth): every forward compositing kernel the library picks on
its own has a DEPTH instantiation (render_fwd.hip, render_rows.hip, render_lanes.hip, render_regions.hip).  Each one is forced in turn and
checked against the float64 dense oracle fed colors_precomp = 1/z and bg = 0; the colour and radii of the same call are bit-identical
to a call without the inverse depth."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

KERNELS = {"quad": "render_forward_kernel", "rows": "render_forward_rows_kernel", "lanes": "render_forward_lanes_kernel",
           "fine": "render_forward_regions_kernel"}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _inputs(sc, mode, dev):
    from das3r_amd import GaussianRasterizationSettings
    kw = {k: v.to(dev) for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()}
    return kw, skw, GaussianRasterizationSettings(**skw)


def _forward(rs, kw, dev, invdepth):
    from das3r_amd import rasterizer
    e = torch.empty(0, device=dev)
    return rasterizer._forward_full(rs, kw["means3D"], kw.get("shs", e), kw.get("colors_precomp", e), kw["opacities"], kw.get("scales", e),
                                    kw.get("rotations", e), kw.get("cov3D_precomp", e), exact=True, invdepth=invdepth)


def _oracle_invdepth(kw, skw):
    """sum_i (1/z_i) alpha_i T_i in float64: the dense oracle's colour with colors_precomp = 1/z (view-space z) and no background."""
    from oracle.dense_oracle import rasterize_dense
    m = kw["means3D"].double()
    V = torch.as_tensor(skw["viewmatrix"]).double().reshape(4, 4)
    z = (torch.cat([m, torch.ones(m.shape[0], 1, dtype=torch.float64, device=m.device)], 1) @ V[:, 2:3]).reshape(-1)
    inv = (1.0 / z.clamp_min(1e-6))[:, None].expand(-1, 3).contiguous()   # (culled splats: never blended, any finite value)
    okw = {k: v for k, v in kw.items() if k not in ("shs", "colors_precomp")}
    oskw = {k: v for k, v in skw.items() if k not in ("prefiltered", "debug")}
    oskw["bg"] = torch.zeros(3, dtype=torch.float64, device=m.device)
    color, _, _ = rasterize_dense(means2D=torch.zeros_like(m), colors_precomp=inv, **okw, **oskw)
    return color[0].cpu()


@pytest.mark.parametrize("name", ["basic_deg3", "long_lists", "deep", "ragged_image", "culled"] + util.CAMERA_VARIANTS)
@pytest.mark.parametrize("kind,binning", [("quad", "radix"), ("rows", "radix"), ("lanes", "radix"), ("fine", "radix"),
                                          ("quad", "local"), ("rows", "local"), ("rows", "seg")])
def test_invdepth_every_forward_kernel_against_the_dense_oracle(name, kind, binning, monkeypatch):
    from das3r_amd import _lib
    sc, mode = util.scene_variant(name)
    monkeypatch.setenv("DAS3R_BINNING", binning)
    monkeypatch.setenv("DAS3R_RENDER", kind)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    base = _forward(rs, kw, dev, False)
    _lib.profile_report()
    _lib.profile_enable(True)
    res = _forward(rs, kw, dev, True)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ran = _lib.profile_report()
    assert ran.get(KERNELS[kind], (0,))[0] == 1 and sum(n for k, (n, _) in ran.items() if k.startswith("render_forward")) == 1, (kind, ran)
    # the colour arithmetic of the DEPTH instantiation is today's: same image, same radii, bit for bit
    assert torch.equal(res[1], base[1]) and torch.equal(res[2], base[2]), name
    inv = res[7]
    assert inv.shape == (1, sc.H, sc.W) and torch.isfinite(inv).all()
    ref = _oracle_invdepth(kw, skw).numpy()
    got = inv[0].double().cpu().numpy()
    scale = max(float(np.abs(ref).max()), 1e-12)
    err = np.abs(got - ref) / scale
    assert (err > 1e-4).mean() < 1e-3 and err.max() < 2e-2, (name, kind, float(err.max()), float((err > 1e-4).mean()))
    assert (got[ref == 0] == 0).all(), "an empty pixel has inverse depth 0 (no background term)"


def _hip_grads(sc, mode, dev, gD, want=True):
    from das3r_amd import GaussianRasterizer
    kw = {k: v.to(dev).clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
    _, _, rs = _inputs(sc, mode, dev)
    means2D = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    res = GaussianRasterizer(rs)(means2D=means2D, **kw, return_invdepth=want)
    loss = (res[0] * sc.dL_dpix.to(dev)).sum() + ((res[2][0] * gD.to(dev)).sum() if want else 0.0)
    loss.backward()
    g = {k: v.grad for k, v in kw.items()}
    g["means2D"] = means2D.grad
    return res, g


def _oracle_grads(sc, mode, gD, dev):
    """d/d(inputs) of <gC, color> + <gD, invdepth> in float64: the colour from one dense call, the inverse depth from a second one with
    colors_precomp = 1/z(means3D) and no background (autograd carries 1/z back to means3D)."""
    from oracle.dense_oracle import rasterize_dense
    kw = {k: v.to(dev).double().clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items() if k not in ("prefiltered", "debug")}
    m2d = torch.zeros(sc.P, 3, dtype=torch.float64, device=dev, requires_grad=True)
    color, _, _ = rasterize_dense(means2D=m2d, **kw, **skw)
    V = torch.as_tensor(skw["viewmatrix"]).double().reshape(4, 4)
    m = kw["means3D"]
    z = (torch.cat([m, torch.ones(m.shape[0], 1, dtype=torch.float64, device=dev)], 1) @ V[:, 2:3]).reshape(-1)
    inv = (1.0 / z.clamp_min(1e-6))[:, None].expand(-1, 3)
    dkw = {k: v for k, v in kw.items() if k not in ("shs", "colors_precomp")}
    dskw = dict(skw, bg=torch.zeros(3, dtype=torch.float64, device=dev))
    depth, _, _ = rasterize_dense(means2D=m2d, colors_precomp=inv, **dkw, **dskw)
    loss = (color * sc.dL_dpix.to(dev).double()).sum() + (depth[0] * gD.to(dev).double()).sum()
    loss.backward()
    g = {k: v.grad for k, v in kw.items()}
    g["means2D"] = m2d.grad
    return g


def _gD(sc, seed=5):
    return torch.randn(sc.H, sc.W, generator=torch.Generator().manual_seed(seed)) * 0.5


@pytest.mark.parametrize("name,bwd", [(n, b) for n in ("basic_deg3", "deep", "culled", "frustum_edge", "portrait_world") for b in ("dpp", "blk", "fine")] + [("long_lists", "dpp")])
def test_invdepth_gradients_against_the_dense_oracle(name, bwd, monkeypatch):
    """L = <gC, color> + <gD, invdepth> through every compositing backward the library picks on its own (forced), against float64 autograd.
    (long_lists on the bucket-parallel blk / fine walks: test_invdepth_gradients_on_long_lists_match_the_colour_path.)"""
    from das3r_amd import _lib
    kernels = {"dpp": "render_backward_kernel", "blk": "render_backward_blk_kernel", "fine": "render_backward_regions_kernel"}
    monkeypatch.setenv("DAS3R_RENDER_BWD", bwd)
    if bwd == "fine":
        monkeypatch.setenv("DAS3R_RENDER", "fine")
    if bwd != "dpp":   # bucket-parallel: "deep" (~4000 entries per tile) starts its buckets from the depth checkpoints
        monkeypatch.setenv("DAS3R_BWD_BUCKETS", "4")
    sc, mode = util.scene_variant(name)
    dev = _dev()
    gD = _gD(sc)
    _lib.profile_report()
    _lib.profile_enable(True)
    _, g = _hip_grads(sc, mode, dev, gD)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ran = _lib.profile_report()
    assert ran.get(kernels[bwd], (0,))[0] == 2 and ran.get("depth_fold_kernel", (0,))[0] == 1, (bwd, ran)   # colour pass + depth pass
    ref = _oracle_grads(sc, mode, gD, dev)
    for k in g:
        util.assert_grad_close(g[k].double().cpu().numpy(), ref[k].cpu().numpy(), f"{name} {bwd} dL/d{k}")


@pytest.mark.parametrize("bwd", ["blk", "fine"])
def test_invdepth_gradients_on_long_lists_match_the_colour_path(bwd, monkeypatch):
    """Long lists, bucket-parallel blk / 2x2-region backward (the depth checkpoints at the bucket starts): the gradient of <gD, invdepth> equals
    that of the library's own colour path fed colors_precomp = (1/z, 0, 0), bg = 0 and dL/dpix = (gD, 0, 0), autograd carrying 1/z to means3D."""
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib
    monkeypatch.setenv("DAS3R_RENDER_BWD", bwd)
    if bwd == "fine":
        monkeypatch.setenv("DAS3R_RENDER", "fine")
    monkeypatch.setenv("DAS3R_BWD_BUCKETS", "4")
    sc, mode = util.scene_variant("long_lists")
    dev = _dev()
    gD = _gD(sc, 11).to(dev)
    kw = {k: v.to(dev).clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
    _, skw, rs = _inputs(sc, mode, dev)
    m2d = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    _lib.profile_report()
    _lib.profile_enable(True)
    c, _, inv = GaussianRasterizer(rs)(means2D=m2d, **kw, return_invdepth=True)
    (inv[0] * gD).sum().backward()
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ran = _lib.profile_report()
    kname = {"blk": "render_backward_blk_kernel", "fine": "render_backward_regions_kernel"}[bwd]
    assert ran.get(kname, (0,))[0] == 2, ran
    got = {k: v.grad for k, v in kw.items() if k != "shs"}
    got["means2D"] = m2d.grad
    assert kw["shs"].grad is None or float(kw["shs"].grad.abs().max()) == 0.0   # (no colour gradient flows)
    # the colour path with the inverse depth as its colour
    kw2 = {k: v.to(dev).clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items() if k != "shs"}
    m = kw2["means3D"]
    V = skw["viewmatrix"].float().reshape(4, 4)
    z = m[:, 0] * V[0, 2] + m[:, 1] * V[1, 2] + m[:, 2] * V[2, 2] + V[3, 2]
    cols = torch.stack([1.0 / z.clamp_min(1e-6), torch.zeros_like(z), torch.zeros_like(z)], 1)
    rs0 = GaussianRasterizationSettings(**dict(skw, bg=torch.zeros(3, device=dev)))
    m2d2 = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    c2, _ = GaussianRasterizer(rs0)(means2D=m2d2, colors_precomp=cols, **kw2)
    (c2[0] * gD).sum().backward()
    assert torch.allclose(c2[0], inv[0], rtol=1e-5, atol=1e-6)
    ref = {k: v.grad for k, v in kw2.items()}
    ref["means2D"] = m2d2.grad
    for k in got:
        util.assert_grad_close(got[k].cpu().numpy(), ref[k].cpu().numpy(), f"long_lists {bwd} depth vs colour path dL/d{k}", tol=1e-5)


def test_invdepth_zero_depth_gradient_equals_the_colour_backward_and_colour_only_is_unchanged(monkeypatch):
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    sc, mode = util.scene_variant("basic_deg3")
    dev = _dev()
    r0, g0 = _hip_grads(sc, mode, dev, None, want=False)
    r1, g1 = _hip_grads(sc, mode, dev, torch.zeros(sc.H, sc.W))
    assert torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1])
    for k in g0:   # the depth pass adds exact zeros
        assert torch.equal(g0[k], g1[k]), k


@pytest.mark.parametrize("name", ["basic_deg3", "deep"])
def test_invdepth_gradients_deterministic(name, monkeypatch):
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    monkeypatch.setenv("DAS3R_BWD_BUCKETS", "4")
    sc, mode = util.scene_variant(name)
    dev = _dev()
    gD = _gD(sc, 7)
    _, a = _hip_grads(sc, mode, dev, gD)
    _, b = _hip_grads(sc, mode, dev, gD)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_scan_backward_has_no_invdepth_form(monkeypatch):
    monkeypatch.setenv("DAS3R_RENDER_BWD", "scan128")
    sc, mode = util.scene_variant("basic_deg3")
    with pytest.raises(RuntimeError, match="no inverse-depth form"):
        _hip_grads(sc, mode, _dev(), _gD(sc))


def test_slices_has_no_invdepth_form(monkeypatch):
    from das3r_amd import _lib
    sc, mode = util.scene_variant("basic_deg3")
    monkeypatch.setenv("DAS3R_RENDER", "slices")
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    _forward(rs, kw, dev, False)   # (colour only: still renders)
    with pytest.raises(RuntimeError, match="slices has no inverse-depth form"):
        _forward(rs, kw, dev, True)
    monkeypatch.delenv("DAS3R_RENDER")
    _lib.reload_switches()
    assert _forward(rs, kw, dev, True)[7].shape == (1, sc.H, sc.W)   # (nothing was left half-done by the refused call)
