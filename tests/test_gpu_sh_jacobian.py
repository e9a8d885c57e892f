"""GPU tests of the SH colour's Jacobian the forward leaves for the backward (das3r_raster_saved.flags bit 2, Layout::g_shjac): with SH at an
active degree >= 2 the per-Gaussian backward reads d(rgb)/d(view direction) from the geometry buffer instead of the SH rows.  Every gradient
is bit-identical to the backward of the same forward with the bit cleared by hand (the SH-row path), the Jacobian planes are really read
when the bit is set (and ignored when it is clear), and the gradients stay within the oracle's bars."""

import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

SHJAC = 4   # das3r_raster_saved.flags bit 2


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _scene(D, M):
    from das3r_amd.synth import make_scene
    sc = make_scene(P=3000, W=128, H=80, focal=100.0, sh_degree=D, seed=40 + D, bg=(0.1, 0.2, 0.3))
    sc.shs[: sc.P // 5, 0, :2] = -3.0   # two channels clamped at 0 for a fifth of the splats
    sc.shs = sc.shs[:, :M].contiguous()
    return sc


def _sh_on(dev, shs, aligned):
    if aligned:
        return shs.to(dev)
    buf = torch.empty(shs.numel() + 1, device=dev)   # 4-byte aligned rows: the unstaged, scalar-load forms
    out = buf[1:].view(shs.shape)
    out.copy_(shs.to(dev))
    return out


def _pre(sc, dev, keep):
    """The raw-parameter form (das3r_raster_in.pre) of the same scene: identity pose, log scales, opacity logits with confidence 1."""
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


def _run(sc, dev, aligned, cov, use_pre, depth):
    from das3r_amd import GaussianRasterizationSettings, rasterizer
    e = torch.empty(0, device=dev)
    rs = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.settings_kwargs().items()})
    means3D, opac = sc.means3D.to(dev), sc.opacities.to(dev)
    shs = _sh_on(dev, sc.shs, aligned)
    scales, rot = (e, e) if cov else (sc.scales.to(dev), sc.rotations.to(dev))
    cov3D = util.cov3d_of(sc).to(dev) if cov else e
    keep = []
    pre = _pre(sc, dev, keep) if use_pre else None
    fw = rasterizer._forward_full(rs, means3D, shs, e, opac, scales, rot, cov3D, exact=True, pre=pre, invdepth=depth)
    I, color, radii, geom, binning, img, cap = fw[:7]
    dD = torch.randn(1, sc.H, sc.W, generator=torch.Generator().manual_seed(5)).to(dev) / (sc.W * sc.H) if depth else None

    def backward(flags):
        assert keep is not None   # (the raw parameters of the pre form live as long as this closure)
        ticket = rasterizer._Capacity(int(cap))
        ticket.check_word, ticket.check_tag, ticket.flags = cap.check_word, cap.check_tag, flags
        g = rasterizer._backward_impl(rs, I, sc.dL_dpix.to(dev), means3D, shs, e, opac, scales, rot, cov3D, geom, binning, img, ticket,
                                      pre=pre, grad_invdepth=dD)
        torch.cuda.synchronize()
        return [t.clone() if t is not None else None for t in g]

    return cap, geom, backward


CASES = [(D, M, aligned, form) for D in range(4) for M in sorted({(D + 1) ** 2, 16}) for aligned in (True, False)
         for form in ("plain", "pre", "depth")] + [(2, 9, True, "cov"), (3, 16, True, "cov")]


@pytest.mark.parametrize("D,M,aligned,form", CASES)
def test_jacobian_backward_is_bit_identical_to_the_sh_row_backward(D, M, aligned, form):
    from das3r_amd import _lib
    dev = _dev()
    sc = _scene(D, M)
    cap, geom, backward = _run(sc, dev, aligned, cov=form == "cov", use_pre=form == "pre", depth=form == "depth")
    assert bool(cap.flags & SHJAC) == (D >= 2)
    with_j = backward(cap.flags)
    rows = backward(cap.flags & ~SHJAC)
    names = ["means2D", "colors", "opacities", "means3D", "cov3D", "shs", "scales", "rotations"]
    for name, a, b in zip(names, with_j, rows):
        assert (a is None) == (b is None), name
        if a is not None:
            assert torch.equal(a, b), f"dL/d{name}: the Jacobian path differs from the SH-row path"
    if D < 2:
        return
    # the planes are what the backward reads: spoilt, they reach dL/dmeans3D with the bit set and nothing with it clear
    off = _lib.layout(sc.P, 0, sc.W, sc.H)["geom_bytes"]
    assert geom.numel() >= off + 36 * sc.P
    geom[off: off + 36 * sc.P].view(torch.float32).fill_(float("nan"))
    assert torch.equal(backward(cap.flags & ~SHJAC)[3], rows[3])
    spoilt = backward(cap.flags)[3]
    bad = torch.isnan(spoilt).any(1)
    assert bad.any() and torch.equal(spoilt[~bad], rows[3][~bad])


@pytest.mark.parametrize("D,M", [(2, 9), (2, 16), (3, 16)])
def test_jacobian_backward_within_the_oracle_bars(D, M):
    dev = _dev()
    sc = _scene(D, M)
    cap, _, backward = _run(sc, dev, True, cov=False, use_pre=False, depth=False)
    assert cap.flags & SHJAC
    g_means2D, _, g_opac, g_means3D, _, g_sh, g_scales, g_rot = backward(cap.flags)
    _, _, ref, _ = util.run_oracle(sc, dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0))
    for name, t in [("means3D", g_means3D), ("opacities", g_opac), ("shs", g_sh), ("scales", g_scales), ("rotations", g_rot),
                    ("means2D", g_means2D)]:
        util.assert_grad_close(t.cpu().numpy(), ref[name], f"D{D} M{M} dL/d{name}")
        util.assert_grad_elementwise(t.cpu().numpy(), ref[name], f"D{D} M{M} dL/d{name}")


def test_chained_jacobian_backward_is_bit_identical_to_the_sh_row_backward():
    """The chained form (das3r_raster_grads.chain: on through the pose pre-transform and the Adam step) at degree 2 with M = 9 — what a
    training run takes at that degree: the parameters, moments, dL/d(confidence) and dL/dshs after the step with the Jacobian read are the
    same bits as after the step from the SH rows (bit 2 cleared), from the same parameters."""
    import math

    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    dev = _dev()
    sc = _scene(2, 9)
    keep = []
    pre = _pre(sc, dev, keep)
    xyz, rot, scaling, logit, conf, _mats = keep
    params = [xyz, rot, scaling, logit]
    start = [p.clone() for p in params]
    e = torch.empty(0, device=dev)
    rs = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.settings_kwargs().items()})
    shs = sc.shs.to(dev)
    I, _, _, geom, binning, img, cap = rasterizer._forward_full(rs, xyz, shs, e, logit, scaling, rot, e, exact=True, pre=pre)
    assert cap.flags & SHJAC

    def step(flags):
        for p, p0 in zip(params, start):
            p.copy_(p0)
        m = [torch.zeros_like(p) for p in params]
        v = [torch.zeros_like(p) for p in params]
        slots = (_lib.AdamSlot * 4)()
        for k in range(4):
            slots[k].param, slots[k].exp_avg, slots[k].exp_avg_sq = params[k].data_ptr(), m[k].data_ptr(), v[k].data_ptr()
            slots[k].step_size, slots[k].bc2_sqrt = 1e-3, math.sqrt(1.0 - 0.999)
        g_conf, g_small = torch.zeros_like(conf), torch.zeros(28, device=dev)
        chain = _lib.Chain()
        chain.g_conf_flat, chain.g_small, chain.slots = g_conf.data_ptr(), g_small.data_ptr(), slots
        chain.beta1, chain.beta2, chain.eps = 0.9, 0.999, 1e-15
        ticket = rasterizer._Capacity(int(cap))
        ticket.check_word, ticket.check_tag, ticket.flags = cap.check_word, cap.check_tag, flags
        g = rasterizer._backward_impl(rs, I, sc.dL_dpix.to(dev), xyz, shs, e, logit, scaling, rot, e, geom, binning, img, ticket,
                                      pre=pre, chain=chain)
        torch.cuda.synchronize()
        return [t.clone() for t in params + m + v] + [g_conf.clone(), g[0].clone(), g[5].clone()]

    with_j, rows = step(cap.flags), step(cap.flags & ~SHJAC)
    assert not torch.equal(with_j[0], start[0])   # (a step was taken)
    for k, (a, b) in enumerate(zip(with_j, rows)):
        assert torch.equal(a, b), k


def test_a_forward_no_backward_follows_leaves_the_jacobian_out(monkeypatch):
    """das3r_raster_saved.flags bit 3 on the way in: an evaluation forward (torch.no_grad, or no input that takes a gradient) does not
    write the planes (bit 2 clear) and renders the same image and radii; the drop-in rasterizer says so exactly when no backward can follow."""
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer, rasterizer
    dev = _dev()
    sc = _scene(3, 16)
    e = torch.empty(0, device=dev)
    rs = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.settings_kwargs().items()})
    kw = dict(means3D=sc.means3D.to(dev), shs=sc.shs.to(dev), opacities=sc.opacities.to(dev), scales=sc.scales.to(dev),
              rotations=sc.rotations.to(dev))
    args = (rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    train = rasterizer._forward_full(*args, exact=True)
    evald = rasterizer._forward_full(*args, exact=True, no_backward=True)
    assert train[6].flags & SHJAC and not evald[6].flags & SHJAC
    assert torch.equal(train[1], evald[1]) and torch.equal(train[2], evald[2])
    seen = []
    real = rasterizer._forward   # (what the autograd function calls; _forward_full is the same call on a plain tuple)
    monkeypatch.setattr(rasterizer, "_forward", lambda *a, **k: seen.append(k.get("no_backward")) or real(*a, **k))
    means2D = torch.zeros(sc.P, 3, device=dev)
    r = GaussianRasterizer(rs)
    with torch.no_grad():
        r(means2D=means2D, **kw)
    r(means2D=means2D, **kw)   # (no input takes a gradient)
    r(means2D=means2D, **{**kw, "shs": kw["shs"].clone().requires_grad_()})
    with torch.no_grad():
        r(means2D=means2D, **{**kw, "shs": kw["shs"].clone().requires_grad_()}, return_invdepth=True)
    assert seen == [True, True, False, True]
