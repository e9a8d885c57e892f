"""GPU tests of the saved-list walk (csrc/render_lists.h) at its edges: tile lists whose length sits ON the batch edge (256 staged entries)
and the half edge (128, the two-half flush of the backward kernels), one short of them and one past them, and two full batches plus one.

Scene: ONE tile (16 x 16, and 13 x 11 for the ragged edge), P Gaussians on the optical axis with an isotropic footprint of 40 .. 60 pixels and
opacity 0.01: every Gaussian covers every pixel with alpha in [0.0095, 0.01] — clear of 1/255 — and T stays above 0.99^513 = 5.8e-3 — clear of
1e-4 — so that no pixel stops early: the tile's list has exactly P entries and every pixel blends all of them.  Both are asserted from the
saved state of every case.

Kernels: composite_features, feature_adjoint, the aux geometry backward with features and coverage in one call, distortion_of forward and
backward.  References: the float64 dense oracle and its autograd (tests/test_gpu_aux.py's and tests/test_gpu_aux_geometry.py's recipes) and
tests/distortion_reference.py.  Bars: tests/util.py's, unchanged.  Every kernel is called twice: the two results are bit-identical."""
import numpy as np
import pytest
import torch

from tests import distortion_reference as dref
from tests import util

pytestmark = pytest.mark.gpu

LENGTHS = [127, 128, 129, 255, 256, 257, 513]
SHAPES = [(16, 16), (13, 11)]
CASES = [(W, H, P) for (W, H) in SHAPES for P in LENGTHS]
IDS = [f"{W}x{H}-P{P}" for W, H, P in CASES]
FOCAL = 16.0
MODE = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
GEOMETRY = ("means3D", "opacities", "scales", "rotations", "means2D")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def edge_scene(W, H, P):
    """P faint Gaussians near the optical axis at distinct depths, each far wider than the one tile of the W x H image (module docstring)."""
    from das3r_amd.synth import make_scene
    sc = make_scene(P=P, W=W, H=H, focal=FOCAL, sh_degree=0, seed=100 + P, opacity=0.01)
    g = torch.Generator().manual_seed(7 * P + W)
    sc.means3D[:, :2] *= 0.1   # within a pixel or so of the image centre
    s_px = 40.0 + 20.0 * torch.rand(P, generator=g)
    sc.scales[:] = (s_px * sc.means3D[:, 2] / FOCAL)[:, None]
    return sc


_CASES = {}


def _case(W, H, P):
    """Per case, computed once and never written to: the scene, its upstream gradients, the forward's saved state, and the float64 references
    {"image" [3, H, W], "adjoint" [P, 3], "aux": {input: gradient}, "D" [H, W], "dist": {input: gradient}} on the host."""
    key = (W, H, P)
    if key in _CASES:
        return _CASES[key]
    from das3r_amd import GaussianRasterizationSettings, rasterizer
    from oracle.dense_oracle import rasterize_dense
    dev = _dev()
    sc = edge_scene(W, H, P)
    gen = torch.Generator().manual_seed(1000 + P)
    F = torch.rand(P, 3, generator=gen)
    G = torch.randn(3, H, W, generator=gen) / float(H * W)
    Ga = torch.randn(1, H, W, generator=gen) / float(H * W)
    Gd = torch.randn(1, H, W, generator=gen) / float(H * W)
    kw = {k: v.to(dev) for k, v in util.raster_inputs(sc, MODE).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, MODE).items()}
    rs = GaussianRasterizationSettings(**skw)
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    state = rasterizer.RasterState.of(res, rs)

    oskw = {k: v for k, v in skw.items() if k not in ("prefiltered", "debug")}
    leaves = {k: kw[k].double().clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
    leaves["means2D"] = torch.zeros(P, 3, dtype=torch.float64, device=dev, requires_grad=True)
    names = list(leaves)
    host = lambda out: {k: (torch.zeros_like(leaves[k]) if g is None else g).cpu() for k, g in zip(names, out)}
    z3 = torch.zeros(3, dtype=torch.float64, device=dev)
    cols = F.to(dev).double().clone().requires_grad_(True)
    img = rasterize_dense(colors_precomp=cols, **leaves, **dict(oskw, bg=z3))[0]
    t = rasterize_dense(colors_precomp=torch.zeros(P, 3, dtype=torch.float64, device=dev), **leaves,
                        **dict(oskw, bg=torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=dev)))[0]
    loss = (img * G.to(dev).double()).sum()
    adjoint = torch.autograd.grad(loss, cols, retain_graph=True)[0].cpu()
    aux = host(torch.autograd.grad(loss + ((1.0 - t[:1]) * Ga.to(dev).double()).sum(), [leaves[k] for k in names], allow_unused=True))
    rest = {k: v for k, v in leaves.items() if k != "opacities"}
    D, _ = dref.distortion_reference(leaves["opacities"], colors_precomp=torch.zeros(P, 3, dtype=torch.float64, device=dev), **rest, **oskw)
    dist = host(torch.autograd.grad((D * Gd[0].to(dev).double()).sum(), [leaves[k] for k in names], allow_unused=True))
    ref = {"image": img.detach().cpu(), "adjoint": adjoint, "aux": aux, "D": D.detach().cpu(), "dist": dist}
    _CASES[key] = dict(sc=sc, kw=kw, rs=rs, state=state, F=F.to(dev), G=G.to(dev).contiguous(), Ga=Ga.to(dev).contiguous(),
                       Gd=Gd.to(dev).contiguous(), ref=ref)
    return _CASES[key]


def _preconditions(c, W, H, P):
    """The tile's range has exactly P entries and the largest n_contrib is P: a scene that fails either is a wrong scene."""
    from das3r_amd import _lib
    state = c["state"]
    assert (W + 15) // 16 == 1 and (H + 15) // 16 == 1, "one tile"
    L = _lib.layout(P, int(state.capacity) if int(state.capacity) > 0 else state.num_rendered, W, H)
    rng = state.img[L["ranges"]:L["ranges"] + 8].view(torch.int32).cpu()
    assert int(rng[1]) - int(rng[0]) == P, f"the tile's range has {int(rng[1]) - int(rng[0])} entries, not {P}"
    n_contrib = state.img[L["n_contrib"]:L["n_contrib"] + 4 * W * H].view(torch.int32)
    assert int(n_contrib.max()) == P, f"the largest n_contrib is {int(n_contrib.max())}, not {P}"


def _twice(call):
    """-> the first result; the second call's is bit-identical, tensor for tensor"""
    a, b = call(), call()
    torch.cuda.synchronize()
    for x, y in zip(a if isinstance(a, (tuple, list)) else (a,), b if isinstance(b, (tuple, list)) else (b,)):
        assert (x is None and y is None) or torch.equal(x, y), "bit-identical from run to run"
    return a


def _rel(got, ref):
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max() / max(np.abs(np.asarray(ref, np.float64)).max(), 1e-300)


def _compare(got, ref, what):
    for k in GEOMETRY:
        assert float(ref[k].abs().max()) > 0, f"{what}: the reference sends nothing to {k}"
        print(f"[{what}] dL/d{k}: max |delta| / max |ref| = {_rel(got[k].double().cpu().numpy(), ref[k].numpy()):.3e} (bar {util.GRAD_REL_TOL})")
        util.assert_grad_close(got[k].cpu().numpy(), ref[k].numpy(), f"{what}: dL/d{k}")


@pytest.mark.parametrize("W,H,P", CASES, ids=IDS)
def test_composite_features(W, H, P):
    from das3r_amd import composite_features
    c = _case(W, H, P)
    _preconditions(c, W, H, P)
    got = _twice(lambda: composite_features(c["state"], c["F"]))
    assert got.shape == (3, H, W)
    d = np.abs(got.double().cpu().numpy() - c["ref"]["image"].numpy())
    print(f"[{W}x{H} P={P}] image: max |delta| {d.max():.3e} (bar {util.COLOR_TOL})")
    util.assert_color_close(got.cpu().numpy(), c["ref"]["image"].numpy(), f"{W}x{H} P={P}: composite_features")


@pytest.mark.parametrize("W,H,P", CASES, ids=IDS)
def test_feature_adjoint(W, H, P):
    from das3r_amd import feature_adjoint
    c = _case(W, H, P)
    _preconditions(c, W, H, P)
    got = _twice(lambda: feature_adjoint(c["state"], c["G"]))
    print(f"[{W}x{H} P={P}] dL_dfeatures: max |delta| / max |ref| = {_rel(got.cpu().numpy(), c['ref']['adjoint'].numpy()):.3e} (bar {util.GRAD_REL_TOL})")
    util.assert_grad_close(got.cpu().numpy(), c["ref"]["adjoint"].numpy(), f"{W}x{H} P={P}: feature_adjoint")


@pytest.mark.parametrize("W,H,P", CASES, ids=IDS)
def test_aux_geometry_backward_with_features_and_coverage(W, H, P):
    from das3r_amd import rasterizer
    c = _case(W, H, P)
    _preconditions(c, W, H, P)
    kw, e = c["kw"], torch.empty(0, device=_dev())
    out = _twice(lambda: rasterizer._aux_backward_impl(c["state"], c["rs"], c["F"], c["G"], c["Ga"], True, kw["means3D"], kw["shs"], e,
                                                        kw["opacities"], kw["scales"], kw["rotations"], e, _fill=float("nan")))
    got = dict(zip(("means2D", "opacities", "means3D", "cov3D_precomp", "scales", "rotations", "features"), out))
    _compare(got, c["ref"]["aux"], f"{W}x{H} P={P} C=3 + coverage")
    util.assert_grad_close(got["features"].cpu().numpy(), c["ref"]["adjoint"].numpy(), f"{W}x{H} P={P}: dL_dfeatures of the same call")


@pytest.mark.parametrize("W,H,P", CASES, ids=IDS)
def test_distortion_forward_and_backward(W, H, P):
    from das3r_amd import rasterizer
    c = _case(W, H, P)
    _preconditions(c, W, H, P)
    kw, e = c["kw"], torch.empty(0, device=_dev())
    D, totals = _twice(lambda: rasterizer._distortion_forward(c["state"], True, _fill=float("nan")))
    assert D.shape == (1, H, W) and float(c["ref"]["D"].max()) > 0
    print(f"[{W}x{H} P={P}] D: max |delta| / max |ref| = {_rel(D[0].cpu().numpy(), c['ref']['D'].numpy()):.3e} (bar {util.GRAD_REL_TOL})")
    util.assert_grad_close(D.reshape(-1).cpu().numpy(), c["ref"]["D"].reshape(-1).numpy(), f"{W}x{H} P={P}: D")   # (no pixel can flip: no allowance)
    out = _twice(lambda: rasterizer._distortion_backward_impl(c["state"], c["rs"], c["Gd"], totals, kw["means3D"], kw["shs"], e, kw["opacities"],
                                                               kw["scales"], kw["rotations"], e, _fill=float("nan")))
    got = dict(zip(("means2D", "opacities", "means3D", "cov3D_precomp", "scales", "rotations"), out))
    _compare(got, c["ref"]["dist"], f"{W}x{H} P={P} distortion")
