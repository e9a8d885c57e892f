"""GPU tests of the normal-consistency regulariser (csrc/normals.hip; include/das3r_raster.h das3r_gaussian_normals_forward / _backward,
das3r_normal_consistency_forward / _backward) and of what is built on it: das3r_amd.gaussian_normals / depth_normals / normal_consistency,
das3r_render(return_normals=, return_normal_consistency=, normal_depth=), OptimParams.normal_weight through train_step.

Reference: tests/normal_reference.py — float64 torch, the definitions taken literally, gradients from autograd; checked itself on the CPU by
tests/test_normal_reference_host.py.  Bars: tests/util.py's, unchanged — util.COLOR_TOL for normal and loss values, util.assert_grad_close at
util.GRAD_REL_TOL for every gradient."""
import copy
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import normal_reference as nref
from tests import util

pytestmark = pytest.mark.gpu

PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
TANFOV = (0.7, 0.45)   # unequal on purpose


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _close(got, ref, what):
    d = float((got.detach().double().cpu() - ref.detach().double().cpu()).abs().max()) if got.numel() else 0.0
    print(f"[{what}] max |delta| = {d:.3e} (bar {util.COLOR_TOL})")
    assert torch.isfinite(got).all(), f"{what}: non-finite value"
    assert d <= util.COLOR_TOL, f"{what}: max |delta| = {d:.3e} > {util.COLOR_TOL}"


def _grad_close(got, ref, what):
    got, ref = got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy()
    scale = max(np.abs(ref).max(), 1e-300) if ref.size else 1.0
    print(f"[{what}] max |delta| / max |ref| = {(np.abs(got - ref).max() / scale if ref.size else 0.0):.3e} (bar {util.GRAD_REL_TOL})")
    util.assert_grad_close(got, ref, what)


# ------------------------------------------------------------------------------------------------------------ 1. per-Gaussian kernels
CAMPOS = (0.25, -0.5, 0.125)   # exactly representable: the hand-made perpendicular row's d is exactly (0, 0, 1)
MIN_COSINE = 1e-4


def _view():
    """A general rotation (and a translation the normals must ignore) as the row-vector view matrix, fp32."""
    g = torch.Generator().manual_seed(17)
    Q = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=g))[0]
    V = torch.eye(4, dtype=torch.float64)
    V[:3, :3] = Q
    V[3, :3] = torch.tensor([0.3, -1.1, 2.0], dtype=torch.float64)
    return V.float().contiguous()


def _rows(P, seed=3):
    """(rotations [P, 4], scales [P, 3], means3D [P, 3], exempt [P] bool) in fp32 on the host.  The hand-made rows come first, as many as fit;
    the means of every row but the exactly perpendicular one are redrawn until |a . d^| >= MIN_COSINE in the float64 reference — a condition
    on the inputs, not a tolerance: no row's flip can then hinge on fp32 rounding."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(P, 4, generator=g)
    s = torch.rand(P, 3, generator=g) * 0.9 + 0.05
    mu = torch.randn(P, 3, generator=g) * 2.0 + torch.tensor([0.0, 0.0, 5.0])
    exempt = torch.zeros(P, dtype=torch.bool)
    unit = lambda v: v / v.norm()
    hand = [
        lambda i: (unit(q[i]) * 0.1, s[i], mu[i]),                                               # a raw quaternion of norm 0.1
        lambda i: (unit(q[i]) * 10.0, s[i], mu[i]),                                              # ... and of norm 10
        lambda i: (q[i], torch.tensor([0.3, 0.3, 0.5]), mu[i]),                                  # two equal smallest scales: k = 0
        lambda i: (q[i], torch.tensor([0.5, 0.3, 0.3]), mu[i]),                                  # ... the other pair: k = 1
        lambda i: (q[i], torch.tensor([0.4, 0.4, 0.4]), mu[i]),                                  # three equal: k = 0
        lambda i: (torch.tensor([1.0, 0.0, 0.0, 0.0]), torch.tensor([0.1, 0.5, 0.5]),            # a = (1, 0, 0), d = (0, 0, 1): a . d = 0 exactly
                   torch.tensor(CAMPOS) + torch.tensor([0.0, 0.0, 1.0])),
    ]
    order = [5, 0, 1, 2, 3, 4]   # (P = 1 runs the perpendicular row)
    for i, h in enumerate(order[:P]):
        q[i], s[i], mu[i] = hand[h](i)
        exempt[i] = h == 5
    campos = torch.tensor(CAMPOS)
    for _ in range(100):
        cos = nref.gaussian_normals(q, s, mu, torch.eye(4), campos)["cosine"]
        bad = (cos.abs() < MIN_COSINE) & ~exempt
        if not bool(bad.any()):
            break
        mu[bad] = torch.randn(int(bad.sum()), 3, generator=g) * 2.0 + torch.tensor([0.0, 0.0, 5.0])
    else:
        raise AssertionError("no admissible rows drawn")
    return q.contiguous(), s.contiguous(), mu.contiguous(), exempt


def _settings(view, campos, H=8, W=8, tan=TANFOV):
    from das3r_amd import GaussianRasterizationSettings
    dev = _dev()
    return GaussianRasterizationSettings(H, W, tan[0], tan[1], torch.zeros(3, device=dev), 1.0, view.to(dev), torch.eye(4, device=dev), 0,
                                         torch.as_tensor(campos, dtype=torch.float32).to(dev), False, False)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 4099])
def test_gaussian_normals_against_the_reference(P):
    from das3r_amd import gaussian_normals, rasterizer
    dev = _dev()
    q, s, mu, exempt = _rows(P)
    view = _view()
    rs = _settings(view, CAMPOS)
    G = torch.randn(P, 3, generator=torch.Generator().manual_seed(5))
    ql = q.double().requires_grad_(True)
    ref = nref.gaussian_normals(ql, s, mu, view, torch.tensor(CAMPOS))
    (ref["normals"] * G.double()).sum().backward()
    # the raw calls, every output filled with NaN first
    nan = float("nan")
    normals, choice = rasterizer._gaussian_normals_forward(rs, q.to(dev), s.to(dev), mu.to(dev), _fill=nan)
    assert choice.dtype == torch.uint8 and torch.equal(choice.cpu().long(), ref["choice"]), "k and flip are the reference's, exactly"
    if P >= 1:
        assert int(choice[0]) == 0 and bool(exempt[0]), "the perpendicular row: a . d = 0 keeps the axis"
        assert torch.equal(normals[0].cpu(), view[0, :3]), "its normal is row 0 of the view rotation, exactly"
    if P >= 6:
        assert [int(c) & 3 for c in choice[3:6]] == [0, 1, 0], "ties take the lowest axis"
    _close(normals, ref["normals"], f"P={P} normals")
    g_rot = rasterizer._gaussian_normals_backward(rs, q.to(dev), choice, G.to(dev), _fill=nan)
    _grad_close(g_rot, ql.grad, f"P={P} dL/drotations")
    # accumulate adds, in one fp32 addition per element
    base = torch.randn(P, 4, generator=torch.Generator().manual_seed(6)).to(dev)
    acc = rasterizer._gaussian_normals_backward(rs, q.to(dev), choice, G.to(dev), out=base.clone(), accumulate=True)
    assert torch.equal(acc, base + g_rot)
    # twice the same bits
    again, choice2 = rasterizer._gaussian_normals_forward(rs, q.to(dev), s.to(dev), mu.to(dev))
    assert torch.equal(again, normals) and torch.equal(choice2, choice)
    assert torch.equal(rasterizer._gaussian_normals_backward(rs, q.to(dev), choice, G.to(dev)), g_rot)
    # the autograd function: the gradient reaches the rotations alone
    leaves = [t.to(dev).requires_grad_(True) for t in (q, s, mu)]
    out = gaussian_normals(rs, *leaves)
    assert torch.equal(out.detach(), normals) and out.requires_grad
    (out * G.to(dev)).sum().backward()
    assert torch.equal(leaves[0].grad, g_rot) and leaves[1].grad is None and leaves[2].grad is None
    with torch.no_grad():
        assert not gaussian_normals(rs, *leaves).requires_grad


def test_gaussian_normals_without_gaussians():
    from das3r_amd import gaussian_normals
    dev = _dev()
    rs = _settings(_view(), CAMPOS)
    q = torch.zeros(0, 4, device=dev, requires_grad=True)
    out = gaussian_normals(rs, q, torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev))
    assert out.shape == (0, 3)
    out.sum().backward()
    assert q.grad.shape == (0, 4)


def test_a_quaternion_without_a_norm_has_no_normal_and_no_gradient():
    from das3r_amd import rasterizer
    dev = _dev()
    rs = _settings(_view(), CAMPOS)
    q = torch.tensor([[0.0, 0.0, 0.0, 0.0], [float("inf"), 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]], device=dev)
    s = torch.tensor([[0.1, 0.2, 0.3]] * 3, device=dev)
    mu = torch.tensor([[0.0, 0.0, 4.0]] * 3, device=dev)
    n, ch = rasterizer._gaussian_normals_forward(rs, q, s, mu)
    assert float(n[:2].abs().max()) == 0.0 and float(n[2].norm()) == pytest.approx(1.0, abs=1e-6)
    g = rasterizer._gaussian_normals_backward(rs, q, ch, torch.ones(3, 3, device=dev))
    assert float(g[:2].abs().max()) == 0.0 and torch.isfinite(g).all()


# ------------------------------------------------------------------------------------------------------------------ 2. image kernels
SHAPES = [(3, 3), (1, 5), (2, 7), (17, 19), (33, 70)]   # (H, W); the kernels' tile is 32 x 8 pixels: 33 x 70 crosses it in both axes


def _image_case(H, W, seed, holes=True):
    """(z, normal, alpha, mask, G) in fp32 on the host: z in [1, 5], smooth plus noise; holes (z = 0), a NaN and an inf on tile borders and in
    halos — the positions that fall inside the image."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = 3.0 + 1.8 * torch.sin(0.31 * xs + 0.2) * torch.cos(0.23 * ys) + 0.03 * torch.randn(H, W, generator=g)
    assert float(z.min()) >= 1.0 and float(z.max()) <= 5.0
    if holes:
        spots = [((7, 31), 0.0), ((8, 32), float("nan")), ((16, 33), float("inf")), ((9, 63), 0.0), ((24, 64), float("nan")), ((31, 40), 0.0),
                 ((15, 1), float("inf")), ((7, 5), 0.0), ((8, 6), float("nan")), ((9, 12), float("inf")), ((4, 17), -2.0), ((0, 3), float("nan")),
                 ((16, 0), 0.0)]
        if H * W > 9:
            for (y, x), v in spots:
                if y < H and x < W:
                    z[y, x] = v
    normal = torch.randn(3, H, W, generator=g)
    alpha = torch.rand(H, W, generator=g)
    mask = torch.rand(H, W, generator=g)
    mask[mask < 0.2] = 0.0
    G = torch.randn(H, W, generator=g)
    return z.contiguous(), normal.contiguous(), alpha.contiguous(), mask.contiguous(), G.contiguous()


def _raw_image_calls(H, W, tan, z, normal, alpha, mask, G, fill=float("nan")):
    """Both library calls on outputs filled with `fill` first -> dict of the seven outputs (on the device)."""
    from das3r_amd import _lib, rasterizer
    dev = _dev()
    lib = _lib.load()
    t = lambda x: None if x is None else x.to(dev).contiguous()
    z, normal, alpha, mask, G = t(z), t(normal), t(alpha), t(mask), t(G)
    new = lambda *s: torch.full(s, fill, dtype=torch.float32, device=dev)
    out = dict(loss=new(H, W), depth_normal=new(3, H, W), g_depth=new(H, W), g_normal=new(3, H, W), g_alpha=new(H, W))
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    stream = rasterizer._stream(dev)
    _lib.check(lib.das3r_normal_consistency_forward(H, W, tan[0], tan[1], p(z), p(normal), p(alpha), p(mask), p(out["loss"]), p(out["depth_normal"]),
                                                    stream), "das3r_normal_consistency_forward")
    _lib.check(lib.das3r_normal_consistency_backward(H, W, tan[0], tan[1], p(z), p(normal), p(mask), p(G), p(out["g_depth"]), p(out["g_normal"]),
                                                     p(out["g_alpha"]), stream), "das3r_normal_consistency_backward")
    torch.cuda.synchronize()
    return out


def _image_reference(tan, z, normal, alpha, mask, G):
    leaves = [x.double().requires_grad_(True) for x in (z, normal, alpha)]
    loss, N, valid = nref.normal_consistency(*leaves, tan[0], tan[1], mask)
    (loss * G.double()).sum().backward()
    return dict(loss=loss.detach(), depth_normal=N.detach(), valid=valid, g_depth=leaves[0].grad, g_normal=leaves[1].grad, g_alpha=leaves[2].grad)


@pytest.mark.parametrize("with_mask", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_image_kernels_against_the_reference(shape, with_mask):
    H, W = shape
    z, normal, alpha, mask, G = _image_case(H, W, seed=40 + H)
    mask = mask if with_mask else None
    ref = _image_reference(TANFOV, z, normal, alpha, mask, G)
    got = _raw_image_calls(H, W, TANFOV, z, normal, alpha, mask, G)
    what = f"{H}x{W} {'mask' if with_mask else 'no mask'}"
    for k, v in got.items():
        assert torch.isfinite(v).all(), f"{what}: {k} is written in full, and no NaN or inf of the depth image reaches it"
    valid = ref["valid"]
    if H < 3 or W < 3:
        assert not bool(valid.any())
        for k, v in got.items():
            assert float(v.abs().max()) == 0.0, f"{what}: no interior pixel, {k} is all zeros"
        return
    assert int(valid.sum()) >= 1
    if (H, W) == (3, 3):
        assert int(valid.sum()) == 1 and bool(valid[1, 1])
    _close(got["loss"], ref["loss"], f"{what} loss")
    _close(got["depth_normal"], ref["depth_normal"], f"{what} depth normal")
    for k in ("g_depth", "g_normal", "g_alpha"):
        assert float(ref[k].abs().max()) > 0
        _grad_close(got[k], ref[k], f"{what} {k}")
    # exact zeros where invalid ...
    inv = ~valid.to(got["loss"].device)
    assert float(got["loss"][inv].abs().max()) == 0.0 and float(got["g_alpha"][inv].abs().max()) == 0.0
    assert float(got["depth_normal"][:, inv].abs().max()) == 0.0 and float(got["g_normal"][:, inv].abs().max()) == 0.0
    # ... and for a depth that no valid stencil reads (its own validity is not a derivative)
    readers = torch.zeros_like(valid)
    readers[:, 1:] |= valid[:, :-1]
    readers[:, :-1] |= valid[:, 1:]
    readers[1:] |= valid[:-1]
    readers[:-1] |= valid[1:]
    unread = ~readers.to(inv.device)
    assert bool(unread.any()) and float(got["g_depth"][unread].abs().max()) == 0.0
    # bit-identical from run to run, whatever the outputs held before
    again = _raw_image_calls(H, W, TANFOV, z, normal, alpha, mask, G, fill=7.0)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{what}: {k} differs between two runs"


PLANES = {"fronto_parallel": ((0.0, 0.0, -1.0), 3.0), "tilted_in_x": ((0.5, 0.0, -1.0), 3.0), "tilted_in_both": ((-0.3, 0.4, -1.0), 2.5)}


@pytest.mark.parametrize("name", list(PLANES))
def test_a_plane_gives_its_own_normal_and_a_zero_loss(name):
    """The plane cases of tests/test_normal_reference_host.py, through the Python surface."""
    from das3r_amd import depth_normals, normal_consistency
    dev = _dev()
    n, dist = PLANES[name]
    n = torch.tensor(n, dtype=torch.float64)
    n = n / n.norm()
    H, W = 11, 41   # two tiles in each axis
    z = nref.plane_depth(H, W, *TANFOV, n, -dist).float()
    assert bool((z > 0).all())
    rs = _settings(torch.eye(4), (0.0, 0.0, 0.0), H, W)
    N = depth_normals(z.to(dev), rs)
    assert N.shape == (3, H, W) and not N.requires_grad
    _close(N[:, 1:-1, 1:-1], n[:, None, None].expand(3, H - 2, W - 2), f"{name}: the depth normal is the plane's")
    assert float(N[:, 0].abs().max()) == 0.0 and float(N[:, -1].abs().max()) == 0.0 and float(N[:, :, 0].abs().max()) == 0.0
    assert float(N[:, :, -1].abs().max()) == 0.0
    if name == "fronto_parallel":
        assert float(N[:2, 1:-1, 1:-1].abs().max()) == 0.0 and float(N[2, 1:-1, 1:-1].max()) < -0.999, "(0, 0, -1): facing the camera"
    alpha = torch.rand(1, H, W, generator=torch.Generator().manual_seed(2)).to(dev)
    loss = normal_consistency(z.to(dev)[None], alpha * n.float().to(dev)[:, None, None], alpha, rs)
    assert loss.shape == (1, H, W) and not loss.requires_grad
    _close(loss, torch.zeros(1, H, W), f"{name}: normal = alpha n costs nothing")


def test_the_python_surface_is_differentiable_and_matches_the_raw_calls():
    from das3r_amd import depth_normals, normal_consistency
    dev = _dev()
    H, W = 17, 19
    z, normal, alpha, mask, G = _image_case(H, W, seed=57)
    raw = _raw_image_calls(H, W, TANFOV, z, normal, alpha, mask, G)
    rs = _settings(torch.eye(4), (0.0, 0.0, 0.0), H, W)
    leaves = [x.to(dev).requires_grad_(True) for x in (z[None], normal, alpha[None])]
    loss = normal_consistency(*leaves, rs, mask=mask.to(dev))
    assert loss.shape == (1, H, W) and loss.requires_grad and torch.equal(loss.detach()[0], raw["loss"])
    (loss * G.to(dev)).sum().backward()
    assert torch.equal(leaves[0].grad[0], raw["g_depth"]) and torch.equal(leaves[1].grad, raw["g_normal"])
    assert torch.equal(leaves[2].grad[0], raw["g_alpha"])
    assert torch.equal(depth_normals(z.to(dev), rs), raw["depth_normal"])
    with torch.no_grad():
        assert torch.equal(normal_consistency(*leaves, rs, mask=mask.to(dev)), loss.detach())


# ------------------------------------------------------------------------------------------------------------------------ 3. end to end
E2E_SCENES = ["depth_ties", "single"]   # 600 Gaussians on 64 x 48 (duplicated splats: tied depths), 1 Gaussian on 48 x 32
_E2E = {}


def _stub_model(sc, dev):
    """What das3r_render reads of a model, as leaves: the scene's tensors are already activated (scales, opacities) and in the camera frame."""
    leaves = {k: getattr(sc, k).to(dev).clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    pc = SimpleNamespace(get_xyz=leaves["means3D"], _xyz=leaves["means3D"], _rotation=leaves["rotations"], get_opacity=leaves["opacities"],
                         get_scaling=leaves["scales"], get_features=leaves["shs"], active_sh_degree=sc.sh_degree, max_sh_degree=3)
    return pc, leaves


def _camera(sc, dev):
    return SimpleNamespace(FoVx=2.0 * math.atan(sc.tanfovx), FoVy=2.0 * math.atan(sc.tanfovy), image_height=sc.H, image_width=sc.W,
                           projection_matrix=sc.projmatrix.to(dev), camera_center=torch.zeros(3, device=dev))


def _e2e_inputs(name):
    """(scene, G [1, H, W], G3 [3, H, W], mask [H, W]) on the host, shared and never written to"""
    if name not in _E2E:
        sc, _ = util.scene_variant(name)
        assert sc.P <= 600 and sc.W <= 64 and sc.H <= 48 and bool(torch.equal(sc.viewmatrix, torch.eye(4)))
        g = torch.Generator().manual_seed(77)
        npix = float(sc.H * sc.W)
        _E2E[name] = (sc, torch.randn(1, sc.H, sc.W, generator=g) / npix, torch.randn(3, sc.H, sc.W, generator=g) / npix,
                      torch.rand(sc.H, sc.W, generator=g))
    return _E2E[name]


POSE = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)   # the identity: the camera frame is the scene's, bit for bit


def _render(name, dev, pipe=PIPE, **kw):
    from das3r_amd.render import das3r_render
    sc = _e2e_inputs(name)[0]
    pc, leaves = _stub_model(sc, dev)
    pkg = das3r_render(_camera(sc, dev), pc, pipe, sc.bg.to(dev), camera_pose=torch.tensor(POSE, device=dev), use_conf=False, **kw)
    return pkg, leaves


def _reference(name, mode, hit, rs, antialiased=False):
    sc, G, G3, mask = _e2e_inputs(name)
    dev = _dev()
    leaves = {k: getattr(sc, k).to(dev).double().clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
    leaves["means2D"] = torch.zeros(sc.P, 3, dtype=torch.float64, device=dev, requires_grad=True)
    settings = dict(tanfovx=float(rs.tanfovx), tanfovy=float(rs.tanfovy), bg=rs.bg, scale_modifier=1.0, viewmatrix=rs.viewmatrix,
                    projmatrix=rs.projmatrix, sh_degree=sc.sh_degree, campos=rs.campos)
    factor = None
    if antialiased:
        from oracle.dense_oracle import rasterize_dense
        from tests.test_gpu_antialiasing import aa_factor
        with torch.no_grad():
            aux = rasterize_dense(colors_precomp=torch.zeros(sc.P, 3, dtype=torch.float64, device=dev), image_height=sc.H, image_width=sc.W,
                                  **{k: v.detach() for k, v in leaves.items()}, **settings)[2]
        factor = aa_factor(aux["conic"])[0][:, None]
    out = nref.end_to_end(leaves, settings, sc.H, sc.W, hit, mode, mask.to(dev), factor)
    return out, leaves


def _settings_of(name, dev):
    from das3r_amd.render import _settings
    sc = _e2e_inputs(name)[0]
    pc, _ = _stub_model(sc, dev)
    return _settings(_camera(sc, dev), pc, PIPE, sc.bg.to(dev), 1.0, dev)


@pytest.mark.parametrize("mode", ["median", "blended"])
@pytest.mark.parametrize("name", E2E_SCENES)
def test_render_against_the_reference(name, mode):
    dev = _dev()
    sc, G, G3, mask = _e2e_inputs(name)
    pkg, leaves = _render(name, dev, return_normal_consistency=True, normal_depth=mode, normal_mask=mask.to(dev), return_median_depth=True)
    assert pkg["normals"].shape == (3, sc.H, sc.W) and pkg["alpha"].shape == (1, sc.H, sc.W) and pkg["normal_consistency"].shape == (1, sc.H, sc.W)
    assert pkg["normals"].requires_grad and pkg["alpha"].requires_grad and pkg["normal_consistency"].requires_grad
    ref, rleaves = _reference(name, mode, pkg["median_hit"], _settings_of(name, dev))
    what = f"{name} {mode}"
    _close(pkg["normals"], ref["normals"], f"{what} normals")
    _close(pkg["alpha"][0], ref["alpha"], f"{what} alpha")
    _close(pkg["normal_depth"][0], ref["z"], f"{what} depth")
    _close(pkg["normal_consistency"][0], ref["loss"], f"{what} loss")
    assert int(ref["valid"].sum()) > 50, "the term is alive on this scene"
    # one scalar over both images; the colour is left out: its gradient is the rasterizer's own business
    ((pkg["normal_consistency"] * G.to(dev)).sum() + (pkg["normals"] * G3.to(dev)).sum()).backward()
    ((ref["loss"] * G[0].to(dev).double()).sum() + (ref["normals"] * G3.to(dev).double()).sum()).backward()
    for k in ("means3D", "opacities", "scales", "rotations"):
        assert leaves[k].grad is not None, f"{what}: no gradient reached {k}"
        assert float(rleaves[k].grad.abs().max()) > 0, k
        _grad_close(leaves[k].grad, rleaves[k].grad, f"{what} dL/d{k}")
    _grad_close(pkg["viewspace_points"].grad, rleaves["means2D"].grad, f"{what} dL/dmeans2D")
    assert leaves["shs"].grad is None or float(leaves["shs"].grad.abs().max()) == 0.0


def test_antialiased_forward_against_the_reference_with_the_factor():
    dev = _dev()
    name = "depth_ties"
    sc, G, G3, mask = _e2e_inputs(name)
    pipe = SimpleNamespace(**vars(PIPE), antialiasing=True)
    with torch.no_grad():
        pkg, _ = _render(name, dev, pipe=pipe, return_normal_consistency=True, normal_mask=mask.to(dev), return_median_depth=True)
    ref, _ = _reference(name, "median", pkg["median_hit"], _settings_of(name, dev), antialiased=True)
    _close(pkg["normals"], ref["normals"], "antialiased normals")
    _close(pkg["normal_consistency"][0], ref["loss"], "antialiased loss")


def test_a_callers_own_features_alongside_are_unchanged():
    dev = _dev()
    name = "depth_ties"
    sc = _e2e_inputs(name)[0]
    feats = torch.randn(sc.P, 5, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        alone, _ = _render(name, dev, features=feats, return_alpha=True)
        both, _ = _render(name, dev, features=feats, return_alpha=True, return_normal_consistency=True)
        only, _ = _render(name, dev, return_normals=True)
    assert torch.equal(alone["features"], both["features"]) and torch.equal(alone["alpha"], both["alpha"]) and torch.equal(alone["render"], both["render"])
    assert torch.equal(only["normals"], both["normals"]) and torch.equal(only["alpha"], alone["alpha"])
    assert "normal_consistency" not in only and "normals" not in alone and "invdepth" not in both


def test_a_covariance_render_is_refused():
    dev = _dev()
    sc = _e2e_inputs("single")[0]
    pc, _ = _stub_model(sc, dev)
    pc.get_covariance = lambda modifier: util.cov3d_of(sc).to(dev)
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=True, convert_SHs_python=False)
    from das3r_amd.render import das3r_render
    with pytest.raises(ValueError, match="has no axes"):
        das3r_render(_camera(sc, dev), pc, pipe, sc.bg.to(dev), camera_pose=torch.tensor(POSE, device=dev), use_conf=False, return_normals=True)


def _kernels_of(fn):
    from das3r_amd import _lib
    _lib.profile_report()
    _lib.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return {k: n for k, (n, _) in _lib.profile_report(raw=True).items()}


def test_with_the_options_off_the_library_calls_are_the_ones_they_were():
    """das3r_render with its defaults launches what a bare GaussianRasterizer call launches, forward and backward — kernel for kernel."""
    from das3r_amd import GaussianRasterizer
    dev = _dev()
    name = "depth_ties"
    sc = _e2e_inputs(name)[0]
    dL = sc.dL_dpix.to(dev)

    def through_render():
        pkg, _ = _render(name, dev)
        assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii"}
        (pkg["render"] * dL).sum().backward()

    def bare():
        _, leaves = _stub_model(sc, dev)
        means2D = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
        out = GaussianRasterizer(_settings_of(name, dev))(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"],
                                                         scales=leaves["scales"], rotations=leaves["rotations"])
        (out[0] * dL).sum().backward()

    through_render(), bare()   # (the shape's first forwards may take another binning path: learn it first)
    a, b = _kernels_of(through_render), _kernels_of(bare)
    assert a == b and a, (a, b)
    assert not any(w in k for k in a for w in ("normal", "aux", "median", "distortion")), a
    on = _kernels_of(lambda: _render(name, dev, return_normal_consistency=True)[0]["normal_consistency"].sum().backward())
    for k in ("gaussian_normals_forward_kernel", "gaussian_normals_backward_kernel<false>", "normal_consistency_forward_kernel",
              "normal_consistency_backward_kernel"):
        assert on.get(k) == 1, (k, on)


def test_render_set_writes_the_normal_maps(tmp_path):
    """What offline --normals does per view, in both render forms: the pair is returned and written as normals/%05d.npy and
    depth_normals/%05d.npy; the two forms agree within the bar (they differ by the rounding of the pose pre-transform); the blended normal is no
    longer than the coverage and the depth normal is a unit vector or zero."""
    from das3r_amd import offline
    from tests.test_gpu_aux import _loaded_model
    model, cams = _loaded_model(W=48, H=32)
    got = {}
    for fused in (True, False):
        pairs, amaps = [], []
        offline.render_set(str(tmp_path / str(fused)), "interp", 7, cams[:2], model, write=True, fused=fused, alpha=amaps, normals=pairs)
        assert len(pairs) == 2
        for idx, ((n, dn), a) in enumerate(zip(pairs, amaps)):
            assert n.shape == (3, 32, 48) and dn.shape == (3, 32, 48) and n.dtype == torch.float32 and not n.requires_grad
            assert bool((n.norm(dim=0) <= a[0] + 1e-5).all()), "a blend of unit vectors with weights that add up to the coverage"
            length = dn.norm(dim=0)
            assert bool(((length == 0) | ((length - 1).abs() < 1e-5)).all()) and float(length.max()) > 0
            for sub, t in (("normals", n), ("depth_normals", dn)):
                arr = np.load(tmp_path / str(fused) / "interp" / "ours_7" / sub / f"{idx:05d}.npy")
                assert arr.shape == (3, 32, 48) and arr.dtype == np.float32 and np.array_equal(arr, t.cpu().numpy())
        got[fused] = pairs
    for (n1, _), (n0, _) in zip(got[True], got[False]):
        _close(n1, n0, "offline normals, fused against the glue form")


# --------------------------------------------------------------------------------------------------------------------------- 4. training
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_term_turns_the_gaussians_to_face_the_surface(seed, monkeypatch):
    """40 fused train steps, once with the weight at 0 and once with it on — set so that the term equals the photometric loss on the first
    step.  The mean normal-consistency over the training views ends strictly lower with the term; with the weight on the direct iteration is
    not entered.  No threshold beyond that comparison."""
    from das3r_amd import fast_step
    from das3r_amd.losses import psnr
    from das3r_amd.model import OptimParams
    from das3r_amd.render import das3r_render
    from das3r_amd.train import build_from_sequence, synthetic_sequence, train_step
    seq = synthetic_sequence(frames=6, W=128, H=80, seed=seed)
    bg = torch.zeros(3, device="cuda")
    entered = []
    direct = fast_step.train_step
    monkeypatch.setattr(fast_step, "train_step", lambda *a, **k: entered.append(1) or direct(*a, **k))

    def mean_term_and_psnr(model, cams):
        with torch.no_grad():
            t, p = [], []
            for c in cams:
                pkg = das3r_render(c, model, PIPE, bg, camera_pose=model.get_RT(c.uid), return_normal_consistency=True)
                t.append(float(pkg["normal_consistency"].mean()))
                p.append(float(psnr(pkg["render"], c.original_image).mean()))
        return sum(t) / len(t), sum(p) / len(p)

    def run(weight):
        model, cams = build_from_sequence(copy.deepcopy(seq))
        opt = OptimParams(iterations=40, normal_weight=weight)
        model.training_setup(opt, fused=True)
        before = mean_term_and_psnr(model, cams)
        del entered[:]
        losses = [float(train_step(model, cams[(it - 1) % len(cams)], opt, it, PIPE, bg, fused=True)[0]) for it in range(1, 41)]
        return losses, len(entered), before, mean_term_and_psnr(model, cams)

    # the weight: the term's value on the first step (the frame's static map as its mask, as train_step passes it) equals the photometric loss's
    model, cams = build_from_sequence(copy.deepcopy(seq))
    opt0 = OptimParams(iterations=40)
    model.training_setup(opt0, fused=True)
    with torch.no_grad():
        first = das3r_render(cams[0], model, PIPE, bg, camera_pose=model.get_RT(cams[0].uid), return_normal_consistency=True,
                             normal_mask=model._conf_static[cams[0].uid].detach())
        term0 = float(first["normal_consistency"].mean())
    photo0 = float(train_step(model, cams[0], opt0, 1, PIPE, bg, fused=True)[0])
    assert term0 > 0 and photo0 > 0
    weight = photo0 / term0

    off_losses, off_direct, (start_term, start_psnr), (off_term, off_psnr) = run(0.0)
    on_losses, on_direct, _, (on_term, on_psnr) = run(weight)
    print(f"seed {seed}: normal weight {weight:.4g} (first step: photometric {photo0:.5f}, mean normal-consistency {term0:.4e})")
    print(f"seed {seed}: mean normal-consistency over the training views: {start_term:.4e} before, {off_term:.4e} after 40 steps without the "
          f"term, {on_term:.4e} with it")
    print(f"seed {seed}: mean training-view PSNR: {start_psnr:.2f} dB before, {off_psnr:.2f} dB without the term, {on_psnr:.2f} dB with it")
    print(f"seed {seed}: steps through the direct iteration: {off_direct} without the term, {on_direct} with it")
    assert on_direct == 0, "with the weight on the direct iteration is not entered"
    assert all(np.isfinite(on_losses)) and all(np.isfinite(off_losses))
    assert on_losses[0] == pytest.approx(2.0 * photo0, rel=1e-3), "the first step's loss is the photometric loss plus a term of the same size"
    assert on_term < off_term
