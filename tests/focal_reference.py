"""The float64 reference of the focal gradient (das3r_raster_backward_focal), shared by tests/test_focal_host.py and tests/test_gpu_focal.py.

s = (s_x, s_y) are log-focal offsets: the forward at s has tanfov e^(-s) and the clip-x / clip-y columns of projmatrix scaled by e^(s).
The unchanged dense oracle takes per-splat tensors, so a per-splat s [P, 2] goes in as tanfovx = tanfovx0 exp(-s[:, 0]) (likewise y) and
means2D[:, :2] = ndc.detach() (exp(s) - 1) — the oracle adds W / 2 means2D to the pixel mean, which is then (u0 - (W - 1) / 2) e^(s) +
(W - 1) / 2.  Autograd on s gives every splat's own contribution c(i); their sum is dL/ds with every discrete decision held fixed (the
oracle's masks are not differentiable, its clamped ray is detached)."""
import math

import torch

from tests import util

RHO_MIN = 2.5e-5


def tiny_scene(seed):
    """The 12-splat scenes on which central differences of the true field-of-view change are clean (no threshold flips at h = 1e-6)."""
    sc = util.make_scene(P=12, W=64, H=48, focal=60.0, sh_degree=1, seed=seed, s_px=(2.0, 6.0))
    return sc, dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)


def aa_factor(conic):
    """f of the dense oracle's conic (A, B, C) = (c, -b, a) / det: the un-dilated entries are a - 0.3 and c - 0.3
    (tests/test_gpu_antialiasing.py builds its reference factor the same way)."""
    A, B, C = conic[:, 0], conic[:, 1], conic[:, 2]
    det = 1.0 / (A * C - B * B)
    a, b, c = C * det, -B * det, A * det
    rho = ((a - 0.3) * (c - 0.3) - b * b) / det
    return torch.sqrt(torch.clamp(rho, min=RHO_MIN))


def _inputs(sc, mode, dev):
    kw = {k: v.to(dev).double() for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items() if k not in ("prefiltered", "debug")}
    return kw, skw


def _loss(kw, skw, m2d, g_pix, g_depth, aa):
    """<g_pix, colour> (+ <g_depth, inverse depth>) of the dense oracle; aa: opacities times the factor of a first call's conic."""
    from oracle.dense_oracle import rasterize_dense
    if aa:
        _, _, aux = rasterize_dense(means2D=m2d, **kw, **skw)
        kw = dict(kw, opacities=kw["opacities"] * aa_factor(aux["conic"])[:, None])
    color, radii, _ = rasterize_dense(means2D=m2d, **kw, **skw)
    loss = (color * g_pix).sum()
    if g_depth is not None:   # the inverse-depth image as tests/test_gpu_invdepth.py's oracle renders it: colour (1/z, 0, 0) over background 0
        V = torch.as_tensor(skw["viewmatrix"]).double().reshape(4, 4).to(kw["means3D"].device)
        m = kw["means3D"]
        z = (torch.cat([m, torch.ones(m.shape[0], 1, dtype=torch.float64, device=m.device)], 1) @ V[:, 2:3]).reshape(-1)
        inv = (1.0 / z.clamp_min(1e-6))[:, None].expand(-1, 3)
        dkw = {k: v for k, v in kw.items() if k not in ("shs", "colors_precomp")}
        depth, _, _ = rasterize_dense(means2D=m2d, colors_precomp=inv, **dkw, **dict(skw, bg=torch.zeros(3, dtype=torch.float64, device=m.device)))
        loss = loss + (depth[0] * g_depth).sum()
    return loss, radii


def per_splat_from(kw, skw, g_pix, g_depth=None, aa=False):
    """per_splat on the oracle's own arguments: kw the float64 tensor inputs (means3D, opacities, shs | colors_precomp, scales + rotations |
    cov3D_precomp), skw the settings without prefiltered / debug, g_pix [3, H, W] (g_depth [H, W]) the upstream gradients, all on one device."""
    dev = kw["means3D"].device
    P = kw["means3D"].shape[0]
    s = torch.zeros(P, 2, dtype=torch.float64, device=dev, requires_grad=True)
    PM0 = torch.as_tensor(skw["projmatrix"]).double().reshape(4, 4).to(dev)
    with torch.no_grad():
        ph = torch.cat([kw["means3D"], torch.ones(P, 1, dtype=torch.float64, device=dev)], 1) @ PM0
        ndc = ph[:, :2] / (ph[:, 3:4] + 1e-7)
    m2d = torch.cat([ndc * (torch.exp(s) - 1.0), torch.zeros(P, 1, dtype=torch.float64, device=dev)], 1)
    k = dict(skw, tanfovx=skw["tanfovx"] * torch.exp(-s[:, 0]), tanfovy=skw["tanfovy"] * torch.exp(-s[:, 1]))
    loss, radii = _loss(kw, k, m2d, g_pix, g_depth, aa)
    loss.backward()
    return s.grad.detach(), radii


def per_splat(sc, mode, dev="cpu", g_depth=None, aa=False):
    """-> (c [P, 2] float64: every splat's dL/ds, radii) of L = <sc.dL_dpix, colour> (+ <g_depth [H, W], inverse depth>)."""
    dev = torch.device(dev)
    kw, skw = _inputs(sc, mode, dev)
    return per_splat_from(kw, skw, sc.dL_dpix.to(dev).double(), None if g_depth is None else g_depth.to(dev).double(), aa)


def true_loss(sc, mode, sx, sy, dev="cpu", g_depth=None, aa=False):
    """L of the true field-of-view change: projmatrix and tanfov rebuilt at (sx, sy), nothing held fixed."""
    dev = torch.device(dev)
    kw, skw = _inputs(sc, mode, dev)
    PM = torch.as_tensor(skw["projmatrix"]).double().reshape(4, 4).clone()
    PM[:, 0] = PM[:, 0] * math.exp(sx)
    PM[:, 1] = PM[:, 1] * math.exp(sy)
    k = dict(skw, projmatrix=PM.to(dev), tanfovx=skw["tanfovx"] * math.exp(-sx), tanfovy=skw["tanfovy"] * math.exp(-sy))
    with torch.no_grad():
        loss, _ = _loss(kw, k, torch.zeros(sc.P, 3, dtype=torch.float64, device=dev), sc.dL_dpix.to(dev).double(),
                        None if g_depth is None else g_depth.to(dev).double(), aa)
    return float(loss)


def central_differences(sc, mode, h, **kw):
    """-> (dL/ds_x, dL/ds_y) by central differences of true_loss at step h."""
    fx = (true_loss(sc, mode, h, 0.0, **kw) - true_loss(sc, mode, -h, 0.0, **kw)) / (2 * h)
    fy = (true_loss(sc, mode, 0.0, h, **kw) - true_loss(sc, mode, 0.0, -h, **kw)) / (2 * h)
    return fx, fy
