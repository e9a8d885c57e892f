"""GPU tests of the ray-distortion regulariser (csrc/render_distort.hip; include/das3r_raster.h das3r_raster_distortion_forward /
das3r_raster_distortion_backward) and of what is built on it: das3r_amd.distortion_of(state, geometry=), das3r_render(return_distortion=),
OptimParams.distortion_weight through train_step.

Reference: tests/distortion_reference.py — the float64 dense oracle's weights rebuilt with autograd, D = 1/2 sum_i sum_j w_i w_j |m_i - m_j|,
m = 1 / depth.  Bars: tests/util.py's, unchanged — util.GRAD_REL_TOL relative to the tensor maximum for the image (a derived sum, not a colour
in [0, 1]: the relative form, with util's threshold-flip allowance) and, without the allowance, for every gradient."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import distortion_reference as dref
from tests import util

pytestmark = pytest.mark.gpu

VARIANTS = ["basic_deg3", "ragged_image", "long_lists", "deep", "culled", "depth_ties", "cov3D_precomp", "single"] + util.CAMERA_VARIANTS
PATHS = [("quad", "radix"), ("rows", "local"), ("rows", "seg"), ("lanes", "radix"), ("fine", "radix")]   # tests/test_gpu_aux_geometry.py's
GEOMETRY = ("means3D", "opacities", "scales", "rotations", "cov3D_precomp", "means2D")
PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _inputs(sc, mode, dev):
    from das3r_amd import GaussianRasterizationSettings
    kw = {k: v.to(dev) for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()}
    return kw, skw, GaussianRasterizationSettings(**skw)


_SCENES, _REF = {}, {}


def _scene(name):
    """(scene, mode, G [1, H, W] ~ N(0, 1) / Npix) on the host — one per variant, shared and never written to"""
    if name not in _SCENES:
        sc, mode = util.scene_variant(name)
        G = torch.randn(1, sc.H, sc.W, generator=torch.Generator().manual_seed(91)) / float(sc.H * sc.W)
        _SCENES[name] = (sc, mode, G)
    return _SCENES[name]


def _reference(name, antialiased=False):
    """{"D": [H, W] float64, "grads": {input: d<G, D>/dinput, float64}} on the host, computed once per (variant, antialiased).  antialiased: the
    oracle fed opacities * f, f from the conic of a first dense call (tests/test_gpu_antialiasing.py's reference)."""
    key = (name, antialiased)
    if key in _REF:
        return _REF[key]
    sc, mode, G = _scene(name)
    dev = _dev()
    leaves = {k: v.to(dev).double().clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items() if k not in ("shs", "colors_precomp")}
    leaves["means2D"] = torch.zeros(sc.P, 3, dtype=torch.float64, device=dev, requires_grad=True)
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items() if k not in ("prefiltered", "debug")}
    colors = torch.zeros(sc.P, 3, dtype=torch.float64, device=dev)
    factor = None
    if antialiased:
        from oracle.dense_oracle import rasterize_dense
        from tests.test_gpu_antialiasing import aa_factor
        factor = aa_factor(rasterize_dense(colors_precomp=colors, **leaves, **skw)[2]["conic"])[0][:, None]
    rest = {k: v for k, v in leaves.items() if k != "opacities"}
    D, _ = dref.distortion_reference(leaves["opacities"], opacity_factor=factor, colors_precomp=colors, **rest, **skw)
    names = list(leaves)
    out = torch.autograd.grad((D * G[0].to(dev).double()).sum(), [leaves[k] for k in names], allow_unused=True)
    _REF[key] = {"D": D.detach().cpu(), "grads": {k: (torch.zeros_like(leaves[k]) if g is None else g).cpu() for k, g in zip(names, out)}}
    return _REF[key]


def _leaves(sc, mode, dev):
    kw = {k: v.to(dev).clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
    kw["means2D"] = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    return kw


def _render(name, dev, **more):
    """One GaussianRasterizer call that keeps its state -> (outputs, leaves, state, AuxGeometry of the leaves)"""
    from das3r_amd import AuxGeometry, GaussianRasterizer
    sc, mode, _ = _scene(name)
    _, _, rs = _inputs(sc, mode, dev)
    kw = _leaves(sc, mode, dev)
    r = GaussianRasterizer(rs, keep_state=True)
    out = r(**kw, **more)
    return out, kw, r.state, AuxGeometry(rs, **kw)


def _rel(got, ref):
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max() / max(np.abs(np.asarray(ref, np.float64)).max(), 1e-300)


def _compare(kw, ref, what):
    for k in GEOMETRY:
        if k in kw:
            got = kw[k].grad
            assert got is not None, f"{what}: no gradient reached {k}"
            print(f"[{what}] dL/d{k}: max |delta| / max |ref| = {_rel(got.double().cpu().numpy(), ref[k].numpy()):.3e} (bar {util.GRAD_REL_TOL})")
            util.assert_grad_close(got.cpu().numpy(), ref[k].numpy(), f"{what}: dL/d{k}")


def _check_forward(name, D, ref, what):
    if name == "single":
        assert float(D.abs().max()) == 0.0, "one Gaussian: every pixel has at most one contributor"
        assert float(ref["D"].abs().max()) == 0.0
        return
    print(f"[{what}] D: max |delta| / max |ref| = {_rel(D.cpu().numpy(), ref['D'].numpy()):.3e} (bar {util.GRAD_REL_TOL}), max D = {float(ref['D'].max()):.4e}")
    util.assert_grad_close(D.reshape(-1).cpu().numpy(), ref["D"].reshape(-1).numpy(), f"{what}: D", flips=True)


def _check_backward(name, kw, ref, what):
    if name == "single":
        for k in GEOMETRY:
            if k in kw:
                assert kw[k].grad is not None and float(kw[k].grad.abs().max()) == 0.0, k
        return
    _compare(kw, ref["grads"], what)
    for k in ("shs", "colors_precomp"):
        if k in kw:
            assert kw[k].grad is None or float(kw[k].grad.abs().max()) == 0.0, "the distortion term sends nothing to the colour"


# ------------------------------------------------------------------------------------------------ 1. against the float64 reference
@pytest.mark.parametrize("name", VARIANTS)
def test_forward_against_the_reference(name):
    from das3r_amd import distortion_of
    sc = _scene(name)[0]
    dev = _dev()
    with torch.no_grad():
        _, _, state, _ = _render(name, dev)
        D = distortion_of(state)
    assert D.shape == (1, sc.H, sc.W) and not D.requires_grad and torch.isfinite(D).all()
    assert float(D.min()) >= 0.0, "the lists are in depth order: every term is >= 0"
    _check_forward(name, D[0], _reference(name), name)


@pytest.mark.parametrize("name", VARIANTS)
def test_backward_against_the_reference(name):
    from das3r_amd import _lib, distortion_of
    sc, _, G = _scene(name)
    dev = _dev()
    _, kw, state, geo = _render(name, dev)
    D = distortion_of(state, geometry=geo)
    assert D.shape == (1, sc.H, sc.W) and D.requires_grad
    assert torch.equal(D.detach(), distortion_of(state)), "the image is distortion_of's own"
    _lib.profile_report()
    _lib.profile_enable(True)
    (D * G.to(dev)).sum().backward()
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ran = _lib.profile_report()
    assert ran.get("render_distortion_backward_kernel", (0,))[0] == 1 and ran.get("distortion_fold_kernel", (0,))[0] == 1, ran
    assert sum(n for k, (n, _) in ran.items() if k.startswith("render_")) == 1, f"one compositing kernel, no second forward: {ran}"
    _check_backward(name, kw, _reference(name), name)


# ------------------------------------------------------------------------------------------- 2. every forward kernel and binning path
def _raw(name, dev, **more):
    """A raw forward of the variant -> (result tuple, state, rs, inputs)"""
    from das3r_amd import rasterizer
    sc, mode, _ = _scene(name)
    kw, _, rs = _inputs(sc, mode, dev)
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], kw.get("shs", e), kw.get("colors_precomp", e), kw["opacities"], kw.get("scales", e),
                                   kw.get("rotations", e), kw.get("cov3D_precomp", e), **more)
    return res, rasterizer.RasterState.of(res, rs), rs, kw


def _raw_backward(state, rs, kw, dev, grad, totals, **more):
    from das3r_amd import rasterizer
    e = torch.empty(0, device=dev)
    out = rasterizer._distortion_backward_impl(state, rs, grad, totals, kw["means3D"], kw.get("shs", e), kw.get("colors_precomp", e), kw["opacities"],
                                               kw.get("scales", e), kw.get("rotations", e), kw.get("cov3D_precomp", e), **more)
    return dict(zip(("means2D", "opacities", "means3D", "cov3D_precomp", "scales", "rotations"), out))


def _raw_check(name, what, ref, **more):
    from das3r_amd import rasterizer
    dev = _dev()
    G = _scene(name)[2].to(dev)
    res, state, rs, kw = _raw(name, dev, **more)
    D, totals = rasterizer._distortion_forward(state, True)
    _check_forward(name, D[0], ref, what)
    got = _raw_backward(state, rs, kw, dev, G.contiguous(), totals)
    for k in GEOMETRY:
        if got.get(k) is not None:
            print(f"[{what}] dL/d{k}: max |delta| / max |ref| = {_rel(got[k].double().cpu().numpy(), ref['grads'][k].numpy()):.3e}")
            util.assert_grad_close(got[k].cpu().numpy(), ref["grads"][k].numpy(), f"{what}: dL/d{k}")


@pytest.mark.parametrize("name", ["basic_deg3", "long_lists"])
@pytest.mark.parametrize("path", PATHS, ids=["-".join(p) for p in PATHS])
def test_forced_kernel_and_binning_pairs(name, path, monkeypatch):
    """The lists differ in provenance, the result must not — within the same bar."""
    monkeypatch.setenv("DAS3R_RENDER", path[0])
    monkeypatch.setenv("DAS3R_BINNING", path[1])
    _raw_check(name, f"{name} {path}", _reference(name))


@pytest.mark.parametrize("name", ["basic_deg3", "deep"])
def test_forward_with_invdepth_leaves_the_same_lists(name):
    _raw_check(name, f"{name} invdepth", _reference(name), invdepth=True)


def test_antialiased_forward_against_the_reference_with_the_factor():
    """The saved opacity carries the factor; the per-Gaussian backward differentiates it as for a colour loss."""
    name = "basic_deg3"
    _raw_check(name, f"{name} antialiased", _reference(name, antialiased=True), antialiasing=True)


# ------------------------------------------------------------------------------------------------------------ 3. existing results do not move
def _small_model(seed=4):
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    seq = synthetic_sequence(frames=3, W=48, H=32, focal=44.0, n_splats=800, seed=seed)
    return build_from_sequence(copy.deepcopy(seq))


MODEL_PARAMS = ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation", "Q", "T")


def test_colour_radii_and_colour_gradients_do_not_move(monkeypatch):
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")   # (the pixel-per-lane backward meets its waves with LDS atomics: bit-equality needs the fixed order)
    from das3r_amd.render import das3r_render
    model, cams = _small_model()
    bg = torch.zeros(3, device="cuda")
    dL = torch.randn(3, 32, 48, generator=torch.Generator().manual_seed(5)).cuda()
    runs = {}
    for on in (False, True):
        for p in MODEL_PARAMS:
            getattr(model, p).grad = None
        pkg = das3r_render(cams[1], model, PIPE, bg, camera_pose=model.get_RT(1), **({"return_distortion": True} if on else {}))
        (pkg["render"] * dL).sum().backward()
        runs[on] = (pkg, {p: getattr(model, p).grad.clone() for p in MODEL_PARAMS if getattr(model, p).grad is not None},
                    pkg["viewspace_points"].grad.clone())
    (p0, g0, m0), (p1, g1, m1) = runs[False], runs[True]
    assert "distortion" not in p0 and p1["distortion"].shape == (1, 32, 48) and p1["distortion"].requires_grad
    assert torch.equal(p0["render"], p1["render"]) and torch.equal(p0["radii"], p1["radii"]) and torch.equal(m0, m1)
    assert set(g0) == set(g1) and "_xyz" in g0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_a_colour_loss_and_a_distortion_loss_through_one_forward_add_up(monkeypatch):
    """Every leaf's gradient is the sum of the two taken separately, within one fp32 addition: autograd adds the two backward calls' results."""
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    from das3r_amd import distortion_of
    name = "basic_deg3"
    sc, _, G = _scene(name)
    dev = _dev()
    dL, G = sc.dL_dpix.to(dev), G.to(dev)
    grads = []
    for terms in ((True, False), (False, True), (True, True)):
        out, kw, state, geo = _render(name, dev)
        D = distortion_of(state, geometry=geo)
        loss = ((out[0] * dL).sum() if terms[0] else 0.0) + ((D * G).sum() if terms[1] else 0.0)
        loss.backward()
        grads.append({k: v.grad for k, v in kw.items()})
    colour, dist, both = grads
    assert dist["shs"] is None or float(dist["shs"].abs().max()) == 0.0
    for k in ("means3D", "opacities", "scales", "rotations", "means2D"):
        assert float(colour[k].abs().max()) > 0 and float(dist[k].abs().max()) > 0, k
        a, b = colour[k].double(), dist[k].double()
        assert bool(((both[k].double() - (a + b)).abs() <= 2.0 ** -23 * (a.abs() + b.abs())).all()), k


# ------------------------------------------------------------------------------------------------------ 4. written in full and reproducible
@pytest.mark.parametrize("name", ["culled", "long_lists", "basic_deg3", "deep"])
def test_everything_is_written_and_reproducible(name):
    from das3r_amd import _lib, rasterizer
    dev = _dev()
    G = _scene(name)[2].to(dev).contiguous()
    res, state, rs, kw = _raw(name, dev)
    nan = float("nan")
    runs = []
    for misalign in (0, 4):   # a scratch that is only 4-byte aligned is accepted
        _lib.poison_lds(0x7FC00000)
        D, totals = rasterizer._distortion_forward(state, True, _fill=nan)
        assert torch.isfinite(D).all() and torch.isfinite(totals).all(), "both planes are written in full"
        _lib.poison_lds(0x7FC00000)
        runs.append((D, totals, _raw_backward(state, rs, kw, dev, G, totals, _fill=nan, _scratch_misalign=misalign)))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "the forward is bit-identical from run to run"
    assert torch.equal(runs[0][0], rasterizer._distortion_forward(state, False, _fill=nan)[0]), "with and without the totals plane"
    unrendered = res[2] == 0
    assert unrendered.any() or name != "culled"
    for k, v in runs[0][2].items():
        if v is None:
            assert k == "cov3D_precomp", k
            continue
        assert torch.isfinite(v).all(), f"dL/d{k}: every element is written, from sums that read nothing unwritten"
        assert torch.equal(v, runs[1][2][k]), f"dL/d{k}: bit-identical from run to run"
        assert (v[unrendered] == 0).all(), f"dL/d{k}: a Gaussian that reached no tile gets an exact zero row"
    for k in ("means3D", "opacities", "scales", "rotations", "means2D"):
        assert float(runs[0][2][k].abs().max()) > 0, k


def test_empty_scene():
    from das3r_amd import AuxGeometry, GaussianRasterizer, distortion_of
    sc, mode = _scene("single")[:2]
    dev = _dev()
    _, _, rs = _inputs(sc, mode, dev)
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)
    kw = dict(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4))
    r = GaussianRasterizer(rs, keep_state=True)
    r(**kw)
    assert float(distortion_of(r.state).abs().max()) == 0.0 and distortion_of(r.state).shape == (1, sc.H, sc.W)
    D = distortion_of(r.state, geometry=AuxGeometry(rs, **kw))
    assert D.shape == (1, sc.H, sc.W) and float(D.detach().abs().max()) == 0.0
    D.sum().backward()
    for k in ("means3D", "means2D", "opacities"):
        assert kw[k].grad is not None and kw[k].grad.shape == kw[k].shape, k


def test_image_smaller_than_a_tile():
    from das3r_amd import AuxGeometry, distortion_of, rasterizer
    from das3r_amd.synth import make_scene
    sc = make_scene(P=40, W=8, H=8, focal=7.0, sh_degree=0, seed=41, s_px=(0.8, 2.5))
    mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    G = (torch.randn(1, 8, 8, generator=torch.Generator().manual_seed(43)) / 64.0).to(dev)
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    state = rasterizer.RasterState.of(res, rs)
    leaves = {k: kw[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
    leaves["means2D"] = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    D = distortion_of(state, geometry=AuxGeometry(rs, shs=kw["shs"], **leaves))
    (D * G).sum().backward()
    ref = {k: v.detach().double().clone().requires_grad_(True) for k, v in leaves.items()}
    oskw = {k: v for k, v in skw.items() if k not in ("prefiltered", "debug")}
    rest = {k: v for k, v in ref.items() if k != "opacities"}
    Dr, _ = dref.distortion_reference(ref["opacities"], colors_precomp=torch.zeros(sc.P, 3, dtype=torch.float64, device=dev), **rest, **oskw)
    (Dr * G[0].double()).sum().backward()
    assert float(Dr.detach().max()) > 0
    util.assert_grad_close(D.detach().reshape(-1).cpu().numpy(), Dr.detach().reshape(-1).cpu().numpy(), "8x8 image: D", flips=True)
    for k in leaves:
        assert float(ref[k].grad.abs().max()) > 0
        util.assert_grad_close(leaves[k].grad.cpu().numpy(), ref[k].grad.cpu().numpy(), f"8x8 image: dL/d{k}")


# --------------------------------------------------------------------------------------------------------------------------- 5. closed form
def test_two_gaussians_on_the_centre_pixel():
    """D = w_1 w_2 (m_1 - m_2) at the pixel both cover, in float64 from the records the forward saved: a wrong sign or a factor of 2 shows here."""
    from das3r_amd import _lib, distortion_of, rasterizer
    from das3r_amd.synth import make_scene
    W, H = 33, 17   # odd: the optical axis meets the centre of pixel (16, 8)
    sc = make_scene(P=2, W=W, H=H, focal=30.0, sh_degree=0, seed=1, s_px=(3.0, 3.0))
    sc.means3D[:] = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 4.0]])
    sc.opacities[:] = torch.tensor([[0.5], [0.4]])
    mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
    dev = _dev()
    kw, _, rs = _inputs(sc, mode, dev)
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    state = rasterizer.RasterState.of(res, rs)
    assert (res[2] > 0).all(), "both are rendered"
    L = _lib.layout(2, int(state.capacity) if int(state.capacity) > 0 else state.num_rendered, W, H)
    rec = lambda off, i: state.geom[L[off] + i * L["splat_stride"]:L[off] + i * L["splat_stride"] + 16].view(torch.float32).double().cpu()
    px, py = 16.0, 8.0
    alpha, m = [], []
    for i in range(2):
        xy, co, rgbd = rec("xy", i), rec("conic_opacity", i), rec("rgbd", i)
        dx, dy = float(xy[0]) - px, float(xy[1]) - py
        power = -0.5 * (float(co[0]) * dx * dx + float(co[2]) * dy * dy) - float(co[1]) * dx * dy
        assert power <= 0.0
        alpha.append(min(0.99, float(co[3]) * float(np.exp(power))))
        m.append(1.0 / float(rgbd[3]))
    assert float(rec("rgbd", 0)[3]) < float(rec("rgbd", 1)[3]) and all(a >= 1.0 / 255.0 for a in alpha)
    w1, w2 = alpha[0], alpha[1] * (1.0 - alpha[0])
    expected = w1 * w2 * (m[0] - m[1])
    assert expected > 0.01, expected
    got = float(distortion_of(state)[0, 8, 16])
    print(f"closed form: kernel {got:.9e}, float64 {expected:.9e}, relative {abs(got - expected) / expected:.3e}")
    assert abs(got - expected) <= 1e-6 * expected


# --------------------------------------------------------------------------------------------------------------------------- 6. end to end
def test_the_unfused_step_carries_the_term():
    """fused=False: the loss train_step returns is the photometric loss plus distortion_weight * mean(D) of the same render, and the step
    leaves the Gaussians elsewhere."""
    from das3r_amd import distortion_of
    from das3r_amd.model import OptimParams
    from das3r_amd.render import das3r_render
    from das3r_amd.train import train_step
    bg = torch.zeros(3, device="cuda")
    results = {}
    for weight in (0.0, 50.0):
        model, cams = _small_model()
        opt = OptimParams(iterations=10, distortion_weight=weight)
        model.training_setup(opt)
        with torch.no_grad():
            pkg = das3r_render(cams[0], model, PIPE, bg, camera_pose=model.get_RT(cams[0].uid), return_state=True)
            mean_d = float(distortion_of(pkg["raster_state"]).mean())
        loss, _, out = train_step(model, cams[0], opt, 1, PIPE, bg, fused=False)
        results[weight] = (float(loss), mean_d, model._xyz.detach().clone(), "distortion" in out)
    (l0, d0, x0, has0), (l1, d1, x1, has1) = results[0.0], results[50.0]
    assert not has0 and has1 and d0 == d1 and d1 > 0
    assert l1 - l0 == pytest.approx(50.0 * d1, rel=1e-4)
    assert not torch.equal(x0, x1)


def test_the_term_pulls_the_copies_along_a_ray_together(monkeypatch):
    """40 fused train steps from one seed, once with the weight at 0 and once with it on — set so that the term equals the photometric loss on
    the first step.  The mean distortion over the training views ends strictly lower with the term; the photometric loss stays finite; with the
    weight on the direct iteration is not entered."""
    from das3r_amd import distortion_of, fast_step
    from das3r_amd.losses import psnr
    from das3r_amd.model import OptimParams
    from das3r_amd.render import das3r_render
    from das3r_amd.train import build_from_sequence, synthetic_sequence, train_step
    seq = synthetic_sequence(frames=6, W=128, H=80)
    bg = torch.zeros(3, device="cuda")
    entered = []
    direct = fast_step.train_step
    monkeypatch.setattr(fast_step, "train_step", lambda *a, **k: entered.append(1) or direct(*a, **k))

    def mean_distortion_and_psnr(model, cams):
        with torch.no_grad():
            d, p = [], []
            for c in cams:
                pkg = das3r_render(c, model, PIPE, bg, camera_pose=model.get_RT(c.uid), return_state=True)
                d.append(float(distortion_of(pkg["raster_state"]).mean()))
                p.append(float(psnr(pkg["render"], c.original_image).mean()))
        return sum(d) / len(d), sum(p) / len(p)

    def run(weight):
        model, cams = build_from_sequence(copy.deepcopy(seq))
        opt = OptimParams(iterations=40, distortion_weight=weight)
        model.training_setup(opt, fused=True)
        del entered[:]
        losses = []
        for it in range(1, 41):
            loss, _, _ = train_step(model, cams[(it - 1) % len(cams)], opt, it, PIPE, bg, fused=True)
            losses.append(float(loss))
        return losses, len(entered), mean_distortion_and_psnr(model, cams)

    # the weight: the term's value on the first step equals the photometric loss's there
    model, cams = build_from_sequence(copy.deepcopy(seq))
    opt0 = OptimParams(iterations=40)
    model.training_setup(opt0, fused=True)
    with torch.no_grad():
        first = das3r_render(cams[0], model, PIPE, bg, camera_pose=model.get_RT(cams[0].uid), return_state=True)
        dist0 = float(distortion_of(first["raster_state"]).mean())
    photo0 = float(train_step(model, cams[0], opt0, 1, PIPE, bg, fused=True)[0])
    assert dist0 > 0 and photo0 > 0
    weight = photo0 / dist0

    off_losses, off_direct, (off_dist, off_psnr) = run(0.0)
    on_losses, on_direct, (on_dist, on_psnr) = run(weight)
    print(f"distortion weight {weight:.4g} (first step: photometric {photo0:.5f}, mean distortion {dist0:.3e})")
    print(f"mean distortion over the training views after 40 steps: {off_dist:.4e} without the term, {on_dist:.4e} with it")
    print(f"mean training-view PSNR after 40 steps: {off_psnr:.2f} dB without the term, {on_psnr:.2f} dB with it")
    assert on_direct == 0, "with the weight on the direct iteration is not entered"
    assert all(np.isfinite(on_losses)) and all(np.isfinite(off_losses))
    assert on_losses[0] == pytest.approx(2.0 * photo0, rel=1e-3), "the first step's loss is the photometric loss plus a term of the same size"
    assert on_dist < off_dist
