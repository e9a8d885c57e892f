"""GPU tests of the aux channels' and the coverage image's gradients to the geometry (csrc/render_aux_bwd.hip; include/das3r_raster.h
das3r_raster_aux_backward) and of what is built on them: GaussianRasterizer(...)(..., features=, return_alpha=, aux_geometry_grad=True),
composite_features(state, features, geometry=), alpha_of(state, geometry=).

References: autograd of the float64 dense oracle fed colors_precomp = three feature columns and bg = 0 (tests/test_gpu_aux.py's recipe), for
the coverage the oracle's 1 - T image (colours 0, bg (1, 0, 0), channel 0); and the library's own colour path (a forward with
colors_precomp = F[:, :3] and bg = 0, das3r_raster_backward with the same upstream gradient).  Bars: tests/util.py's, unchanged, no flips
allowance.  The coverage is never taken from a constant feature column (ill-conditioned in fp32 on `deep`: docs/ledger.md (ck))."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

VARIANTS = ["basic_deg3", "ragged_image", "long_lists", "deep", "culled", "depth_ties", "cov3D_precomp", "single"] + util.CAMERA_VARIANTS
PATHS = [("quad", "radix"), ("rows", "local"), ("rows", "seg"), ("lanes", "radix"), ("fine", "radix")]   # tests/test_gpu_aux.py's


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _inputs(sc, mode, dev):
    from das3r_amd import GaussianRasterizationSettings
    kw = {k: v.to(dev) for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()}
    return kw, skw, GaussianRasterizationSettings(**skw)


def _features(P, width=8, seed=77):
    return torch.rand(P, width, generator=torch.Generator().manual_seed(seed))


def _grad_image(sc, width=8, seed=78):
    """G ~ N(0, 1) / Npix"""
    return torch.randn(width, sc.H, sc.W, generator=torch.Generator().manual_seed(seed)) / float(sc.H * sc.W)


_SCENES, _ORACLE = {}, {}
GEOMETRY = ("means3D", "opacities", "scales", "rotations", "cov3D_precomp", "means2D")


def _scene(name):
    """(scene, mode, features [P, 8], G [8, H, W], G_alpha [1, H, W]) on the host — one per variant, shared and never written to"""
    if name not in _SCENES:
        sc, mode = util.scene_variant(name)
        _SCENES[name] = (sc, mode, _features(sc.P), _grad_image(sc), _grad_image(sc, 1, seed=79))
    return _SCENES[name]


def _oracle(name):
    """{"C1" | "C3" | "C8" | "alpha": {input: float64 gradient on the host}} — autograd of the dense oracle for <G[:C], image of F[:, :C]> and
    for <G_alpha, 1 - T>, with respect to the geometry inputs and means2D.  Three oracle channels at a time; the gradients of C = 8 are the
    sums of its three chunks'.  Computed once per variant."""
    if name in _ORACLE:
        return _ORACLE[name]
    from oracle.dense_oracle import rasterize_dense
    sc, mode, F, G, Ga = _scene(name)
    dev = _dev()
    leaves = {k: v.to(dev).double().clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items() if k not in ("shs", "colors_precomp")}
    leaves["means2D"] = torch.zeros(sc.P, 3, dtype=torch.float64, device=dev, requires_grad=True)
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items() if k not in ("prefiltered", "debug")}
    Fd, Gd = F.to(dev).double(), G.to(dev).double()

    def grads_of(colors, bg, weight):
        """d<weight, image>/d leaves"""
        img = rasterize_dense(colors_precomp=colors, **leaves, **dict(skw, bg=bg))[0]
        names = list(leaves)
        out = torch.autograd.grad((img * weight).sum(), [leaves[k] for k in names], allow_unused=True)
        return {k: (torch.zeros_like(leaves[k]) if g is None else g).cpu() for k, g in zip(names, out)}

    zero3 = torch.zeros(3, dtype=torch.float64, device=dev)
    add = lambda a, b: {k: a[k] + b[k] for k in a}
    first = Fd[:, [0, 1, 2]].contiguous()
    c1 = grads_of(first, zero3, torch.cat([Gd[:1], torch.zeros_like(Gd[:2])], 0))
    c3 = grads_of(first, zero3, Gd[:3])
    mid = grads_of(Fd[:, [3, 4, 5]].contiguous(), zero3, Gd[3:6])
    last = grads_of(Fd[:, [6, 7, 7]].contiguous(), zero3, torch.cat([Gd[6:8], torch.zeros_like(Gd[:1])], 0))
    # coverage: colours 0 over bg (1, 0, 0) leave T in channel 0; 1 - T takes the sign
    w = torch.cat([-Ga.to(dev).double(), torch.zeros(2, sc.H, sc.W, dtype=torch.float64, device=dev)], 0)
    alpha = grads_of(torch.zeros(sc.P, 3, dtype=torch.float64, device=dev), torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=dev), w)
    _ORACLE[name] = {"C1": c1, "C3": c3, "C8": add(add(c3, mid), last), "alpha": alpha}
    return _ORACLE[name]


def _leaves(sc, mode, dev):
    kw = {k: v.to(dev).clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
    kw["means2D"] = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    return kw


def _render(name, C_, alpha, dev, on=True, **more):
    """One GaussianRasterizer call on the variant's leaves -> (outputs, leaves, features leaf or None)"""
    from das3r_amd import GaussianRasterizer
    sc, mode, F, _, _ = _scene(name)
    _, _, rs = _inputs(sc, mode, dev)
    kw = _leaves(sc, mode, dev)
    feats = F[:, :C_].contiguous().to(dev).requires_grad_(True) if C_ else None
    extra = dict(more)
    if feats is not None:
        extra["features"] = feats
    if alpha:
        extra["return_alpha"] = True
    if on:
        extra["aux_geometry_grad"] = True
    return GaussianRasterizer(rs)(**kw, **extra), kw, feats


def _compare(kw, ref, what):
    for k in GEOMETRY:
        if k in kw:
            got = kw[k].grad
            assert got is not None, f"{what}: no gradient reached {k}"
            rel = np.abs(got.double().cpu().numpy() - ref[k].numpy()).max() / max(np.abs(ref[k].numpy()).max(), 1e-300)
            print(f"[{what}] dL/d{k}: max |delta| / max |ref| = {rel:.3e} (bar {util.GRAD_REL_TOL})")
            util.assert_grad_close(got.cpu().numpy(), ref[k].numpy(), f"{what}: dL/d{k}")


# ------------------------------------------------------------------------------------------------ 1. against autograd of the float64 dense oracle
@pytest.mark.parametrize("C_", [1, 3, 8])
@pytest.mark.parametrize("name", VARIANTS)
def test_feature_loss_against_the_dense_oracle(name, C_):
    sc, mode, F, G, _ = _scene(name)
    dev = _dev()
    out, kw, feats = _render(name, C_, False, dev)
    assert len(out) == 3 and out[2].shape == (C_, sc.H, sc.W)
    (out[2] * G[:C_].to(dev)).sum().backward()
    _compare(kw, _oracle(name)[f"C{C_}"], f"{name} C={C_}")
    for k in ("shs", "colors_precomp"):
        if k in kw:
            assert kw[k].grad is None or float(kw[k].grad.abs().max()) == 0.0, "an aux loss sends nothing to the colour"


@pytest.mark.parametrize("name", VARIANTS)
def test_coverage_loss_alone_against_the_dense_oracle(name):
    """C = 0: the direct form T_final / (1 - alpha_k)"""
    sc, mode, _, _, Ga = _scene(name)
    dev = _dev()
    out, kw, _ = _render(name, 0, True, dev)
    assert len(out) == 3 and out[2].shape == (1, sc.H, sc.W) and out[2].requires_grad
    (out[2] * Ga.to(dev)).sum().backward()
    _compare(kw, _oracle(name)["alpha"], f"{name} coverage")


@pytest.mark.parametrize("name", VARIANTS)
def test_features_and_coverage_in_one_call_against_the_dense_oracle(name):
    from das3r_amd import _lib
    sc, mode, _, G, Ga = _scene(name)
    dev = _dev()
    out, kw, feats = _render(name, 3, True, dev)
    loss = (out[2] * G[:3].to(dev)).sum() + (out[3] * Ga.to(dev)).sum()
    _lib.profile_report()
    _lib.profile_enable(True)
    loss.backward()
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ran = _lib.profile_report()
    assert ran.get("render_aux_backward_kernel", (0,))[0] == 1, ran   # ONE library call for both upstream gradients
    assert not any(k.startswith("render_forward") or k.startswith("render_aux_adjoint") or k.startswith("render_backward") for k in ran), ran
    o = _oracle(name)
    _compare(kw, {k: o["C3"][k] + o["alpha"][k] for k in o["C3"]}, f"{name} C=3 + coverage")
    assert feats.grad is not None and float(feats.grad.abs().max()) > 0


# --------------------------------------------------------------------------------------------------- 2. against the library's own colour path
def _raw_forward(rs, kw, dev, colors, **more):
    from das3r_amd import rasterizer
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], e, colors, kw["opacities"], kw.get("scales", e), kw.get("rotations", e), kw.get("cov3D_precomp", e),
                                   **more)
    return res, rasterizer.RasterState.of(res, rs)


def _raw_aux_backward(state, rs, kw, dev, feats, G, Ga, want_features=True, colors=None, **more):
    from das3r_amd import rasterizer
    e = torch.empty(0, device=dev)
    out = rasterizer._aux_backward_impl(state, rs, feats, G, Ga, want_features, kw["means3D"], e if colors is not None else kw.get("shs", e),
                                        colors if colors is not None else e, kw["opacities"], kw.get("scales", e), kw.get("rotations", e),
                                        kw.get("cov3D_precomp", e), **more)
    return dict(zip(("means2D", "opacities", "means3D", "cov3D_precomp", "scales", "rotations", "features"), out))


def _self_check(name, dev, what, **more):
    """das3r_raster_aux_backward on a forward with colors_precomp = F[:, :3] and bg = 0 against das3r_raster_backward with the same G: the
    geometry and means2D gradients, and dL_dfeatures against dL_dcolors_precomp and against feature_adjoint."""
    from das3r_amd import GaussianRasterizationSettings, _lib, feature_adjoint, rasterizer
    sc, mode, F, G, _ = _scene(name)
    kw, skw, _ = _inputs(sc, mode, dev)
    rs = GaussianRasterizationSettings(**dict(skw, bg=torch.zeros(3, device=dev)))
    cols = F[:, :3].contiguous().to(dev)
    G3 = G[:3].contiguous().to(dev)
    res, state = _raw_forward(rs, kw, dev, cols, **more)
    e = torch.empty(0, device=dev)
    ref = rasterizer._backward_impl(rs, res[0], G3, kw["means3D"], e, cols, kw["opacities"], kw.get("scales", e), kw.get("rotations", e),
                                    kw.get("cov3D_precomp", e), res[3], res[4], res[5], res[6])
    ref = dict(zip(("means2D", "features", "opacities", "means3D", "cov3D_precomp", "shs", "scales", "rotations"), ref))
    _lib.profile_report()
    _lib.profile_enable(True)
    got = _raw_aux_backward(state, rs, kw, dev, cols, G3, None, colors=cols)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ran = _lib.profile_report()
    assert ran.get("render_aux_backward_kernel", (0,))[0] == 1 and ran.get("aux_gather_kernel", (0,))[0] == 1, ran
    assert sum(n for k, (n, _) in ran.items() if k.startswith("render_")) == 1, f"one compositing kernel, no second forward: {ran}"
    for k in ("means3D", "opacities", "scales", "rotations", "means2D", "features"):
        util.assert_grad_close(got[k].cpu().numpy(), ref[k].cpu().numpy(), f"{what}: dL/d{k} vs the colour path")
    util.assert_grad_close(got["features"].cpu().numpy(), feature_adjoint(state, G3).cpu().numpy(), f"{what}: dL_dfeatures vs feature_adjoint")


@pytest.mark.parametrize("name", ["basic_deg3", "long_lists"])
@pytest.mark.parametrize("path", [None] + PATHS, ids=["default"] + ["-".join(p) for p in PATHS])
def test_against_the_librarys_own_colour_path(name, path, monkeypatch):
    if path is not None:
        monkeypatch.setenv("DAS3R_RENDER", path[0])
        monkeypatch.setenv("DAS3R_BINNING", path[1])
    _self_check(name, _dev(), f"{name} {path}")


@pytest.mark.parametrize("name", ["basic_deg3", "long_lists"])
def test_antialiased_forward_against_its_own_colour_path(name):
    """The antialiasing factor's derivative is the per-Gaussian backward's, applied as for a colour loss."""
    _self_check(name, _dev(), f"{name} antialiased", antialiasing=True)


@pytest.mark.parametrize("name", ["basic_deg3", "deep"])
def test_forward_with_invdepth_against_its_own_colour_path(name):
    _self_check(name, _dev(), f"{name} invdepth", invdepth=True)


# ------------------------------------------------------------------------------------------------------------ 3. dL_dfeatures from the same call
@pytest.mark.parametrize("C_", [1, 3, 8])
@pytest.mark.parametrize("name", ["basic_deg3", "deep", "culled", "long_lists"])
def test_feature_gradient_of_the_same_call_is_the_adjoints(name, C_):
    from das3r_amd import feature_adjoint
    sc, mode, F, G, Ga = _scene(name)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    e = torch.empty(0, device=dev)
    from das3r_amd import rasterizer
    res = rasterizer._forward_full(rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    state = rasterizer.RasterState.of(res, rs)
    f, g = F[:, :C_].contiguous().to(dev), G[:C_].contiguous().to(dev)
    got = _raw_aux_backward(state, rs, kw, dev, f, g, Ga.to(dev))["features"]   # (the coverage term sends nothing to the features)
    util.assert_grad_close(got.cpu().numpy(), feature_adjoint(state, g).cpu().numpy(), f"{name} C={C_}: dL_dfeatures vs feature_adjoint")
    assert _raw_aux_backward(state, rs, kw, dev, f, g, None, want_features=False)["features"] is None


# ------------------------------------------------------------------------------------------------------ 4. written in full and reproducible
@pytest.mark.parametrize("C_", [0, 1, 3, 8])
@pytest.mark.parametrize("name", ["culled", "long_lists", "basic_deg3", "deep"])
def test_everything_is_written_and_reproducible(name, C_):
    from das3r_amd import _lib, rasterizer
    sc, mode, F, G, Ga = _scene(name)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    state = rasterizer.RasterState.of(res, rs)
    f = F[:, :C_].contiguous().to(dev) if C_ else None
    g = G[:C_].contiguous().to(dev) if C_ else None
    runs = []
    for misalign in (0, 4):   # a scratch that is only 4-byte aligned is accepted
        _lib.poison_lds(0x7FC00000)
        runs.append(_raw_aux_backward(state, rs, kw, dev, f, g, Ga.to(dev), want_features=C_ > 0, _fill=float("nan"), _scratch_misalign=misalign))
    torch.cuda.synchronize()
    unrendered = res[2] == 0
    assert unrendered.any() or name != "culled"
    for k, v in runs[0].items():
        if v is None:
            assert k in ("cov3D_precomp", "features"), k
            continue
        assert torch.isfinite(v).all(), f"dL/d{k}: every element is written, from sums that read nothing unwritten"
        assert torch.equal(v, runs[1][k]), f"dL/d{k}: bit-identical from run to run"
        assert (v[unrendered] == 0).all(), f"dL/d{k}: a Gaussian that reached no tile gets an exact zero row"
    for k in ("means3D", "opacities", "scales", "rotations", "means2D"):
        assert float(runs[0][k].abs().max()) > 0, k


# -------------------------------------------------------------------------------------------------------------------- 5. nothing existing moves
@pytest.mark.parametrize("name", ["basic_deg3", "culled"])
def test_colour_radii_and_colour_gradients_do_not_move(name, monkeypatch):
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")   # (the pixel-per-lane backward meets its waves with LDS atomics: bit-equality needs the fixed order)
    sc = _scene(name)[0]
    dev = _dev()
    dL = sc.dL_dpix.to(dev)
    outs = {}
    for on in (False, True):
        out, kw, feats = _render(name, 4, True, dev, on=on)
        assert len(out) == 4
        (out[0] * dL).sum().backward()
        outs[on] = (out, kw, feats)
    (o0, k0, f0), (o1, k1, f1) = outs[False], outs[True]
    assert torch.equal(o0[0], o1[0]) and torch.equal(o0[1], o1[1]) and torch.equal(o0[2], o1[2]) and torch.equal(o0[3], o1[3])
    for k in k0:
        assert torch.equal(k0[k].grad, k1[k].grad), k
    assert f0.grad is None and f1.grad is None, "a colour loss sends nothing to the features"
    assert o1[2].requires_grad and o1[3].requires_grad and not o0[3].requires_grad


def test_with_the_keyword_off_a_feature_loss_reaches_the_features_alone():
    name = "basic_deg3"
    sc, mode, F, G, _ = _scene(name)
    dev = _dev()
    out, kw, feats = _render(name, 3, False, dev, on=False)
    (out[2] * G[:3].to(dev)).sum().backward()
    assert feats.grad is not None and float(feats.grad.abs().max()) > 0
    for k, v in kw.items():
        assert v.grad is None or float(v.grad.abs().max()) == 0.0, k


# ------------------------------------------------------------------------------------------------------------------- 6. autograd composition
def test_three_losses_through_one_forward_add_up(monkeypatch):
    """Colour, feature and coverage losses through ONE GaussianRasterizer call: every leaf's gradient is the sum of the three taken separately.
    The combined aux gradient is one kernel pass over both upstream gradients, not a sum of rounded results, so the two sides are two fp32
    evaluations of the same sums: they are held to the bar every fp32 gradient here is held to (util.GRAD_REL_TOL), relative to the largest
    element of the summed reference."""
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    name = "basic_deg3"
    sc, mode, F, G, Ga = _scene(name)
    dev = _dev()
    dL, G3, Ga = sc.dL_dpix.to(dev), G[:3].to(dev), Ga.to(dev)
    terms = (lambda o: (o[0] * dL).sum(), lambda o: (o[2] * G3).sum(), lambda o: (o[3] * Ga).sum())
    separate = []
    for term in terms:
        out, kw, feats = _render(name, 3, True, dev)
        term(out).backward()
        separate.append({**{k: v.grad for k, v in kw.items()}, "features": feats.grad})
    assert separate[0]["features"] is None and separate[2]["features"] is None and separate[1]["shs"] is None
    for i in range(3):
        assert float(separate[i]["means2D"].abs().max()) > 0, "means2D.grad carries all three"
    out, kw, feats = _render(name, 3, True, dev)
    loss = terms[0](out) + terms[1](out) + terms[2](out)
    loss.backward(retain_graph=True)
    got = {**{k: v.grad.clone() for k, v in kw.items()}, "features": feats.grad.clone()}
    for k, v in got.items():
        parts = [s[k].double() for s in separate if s[k] is not None]
        util.assert_grad_close(v.cpu().numpy(), sum(parts).cpu().numpy(), f"one forward, three losses: dL/d{k}")
    loss.backward()   # a second backward over the retained graph: every leaf doubles
    for k, v in kw.items():
        util.assert_grad_close(v.grad.cpu().numpy(), (2.0 * got[k].double()).cpu().numpy(), f"second backward: dL/d{k}")


# ------------------------------------------------------------------------------------------------------------------------------- 7. edges
def test_empty_scene():
    from das3r_amd import GaussianRasterizer
    sc, mode = _scene("single")[:2]
    dev = _dev()
    _, _, rs = _inputs(sc, mode, dev)
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)
    kw = dict(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4))
    feats = z(0, 5)
    color, radii, fimg, alpha = GaussianRasterizer(rs)(**kw, features=feats, return_alpha=True, aux_geometry_grad=True)
    assert fimg.shape == (5, sc.H, sc.W) and alpha.shape == (1, sc.H, sc.W) and radii.numel() == 0
    assert float(fimg.detach().abs().max()) == 0.0 and float(alpha.detach().abs().max()) == 0.0
    (fimg.sum() + alpha.sum()).backward()
    for k in ("means3D", "means2D", "opacities"):
        assert kw[k].grad is not None and kw[k].grad.shape == kw[k].shape, k
    assert feats.grad.shape == (0, 5)


def test_image_smaller_than_a_tile():
    from das3r_amd import AuxGeometry, alpha_of, composite_features, rasterizer
    from das3r_amd.synth import make_scene
    from oracle.dense_oracle import rasterize_dense
    sc = make_scene(P=40, W=7, H=5, focal=6.0, sh_degree=0, seed=41, s_px=(0.8, 2.5))
    mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    F, G, Ga = _features(sc.P, 3, seed=42), _grad_image(sc, 3, seed=43), _grad_image(sc, 1, seed=44)
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    state = rasterizer.RasterState.of(res, rs)
    # from a kept state: composite_features / alpha_of with the forward's settings and tensors
    leaves = {k: kw[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
    leaves["means2D"] = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    geo = AuxGeometry(rs, shs=kw["shs"], **leaves)
    img, alpha = composite_features(state, F.to(dev), geometry=geo), alpha_of(state, geometry=geo)
    assert img.shape == (3, 5, 7) and alpha.shape == (1, 5, 7)
    ((img * G.to(dev)).sum() + (alpha * Ga.to(dev)).sum()).backward()
    ref = {k: v.detach().double().clone().requires_grad_(True) for k, v in leaves.items()}
    oskw = {k: v for k, v in skw.items() if k not in ("prefiltered", "debug")}
    z3 = torch.zeros(3, dtype=torch.float64, device=dev)
    a = rasterize_dense(colors_precomp=F.to(dev).double(), **ref, **dict(oskw, bg=z3))[0]
    t = rasterize_dense(colors_precomp=torch.zeros(sc.P, 3, dtype=torch.float64, device=dev), **ref,
                        **dict(oskw, bg=torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=dev)))[0]
    ((a * G.to(dev).double()).sum() + ((1.0 - t[:1]) * Ga.to(dev).double()).sum()).backward()
    for k in leaves:
        assert float(ref[k].grad.abs().max()) > 0
        util.assert_grad_close(leaves[k].grad.cpu().numpy(), ref[k].grad.cpu().numpy(), f"7x5 image: dL/d{k}")


def test_eight_channels_on_a_ragged_image_from_a_kept_state():
    """C = 8 on ragged_image through composite_features(state, features, geometry=) (the rasterizer call's form is in test 1)."""
    from das3r_amd import AuxGeometry, composite_features, rasterizer
    name = "ragged_image"
    sc, mode, F, G, _ = _scene(name)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    state = rasterizer.RasterState.of(res, rs)
    leaves = {k: kw[k].clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
    leaves["means2D"] = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    img = composite_features(state, F.to(dev), geometry=AuxGeometry(rs, shs=kw["shs"], **leaves))
    assert torch.equal(img.detach(), composite_features(state, F.to(dev))), "the image is composite_features' own"
    (img * G.to(dev)).sum().backward()
    _compare(leaves, _oracle(name)["C8"], f"{name} C=8 from a kept state")


# --------------------------------------------------------------------------------------------------------------------------- 8. end to end
def _mask_run(on, steps=30):
    from das3r_amd import GaussianRasterizer
    sc, mode = _scene("basic_deg3")[:2]
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    mask = (torch.arange(sc.W, device=dev)[None, None, :] < sc.W / 2).float().expand(1, sc.H, sc.W)   # the half-plane x < W / 2
    means3D = kw["means3D"].clone().requires_grad_(True)
    log_scales = kw["scales"].log().clone().requires_grad_(True)
    logit = torch.logit(kw["opacities"].clamp(1e-4, 1 - 1e-4)).clone().requires_grad_(True)
    params = [means3D, log_scales, logit]
    opt = torch.optim.Adam(params, lr=0.02)
    losses, reached = [], True
    for step in range(steps + 1):   # the loss before every step, and once more after the last
        extra = {"aux_geometry_grad": True} if on else {}
        out = GaussianRasterizer(rs)(means3D=means3D, means2D=torch.zeros(sc.P, 3, device=dev, requires_grad=True), opacities=torch.sigmoid(logit),
                                     shs=kw["shs"], scales=log_scales.exp(), rotations=kw["rotations"], return_alpha=True, **extra)
        loss = ((out[2] - mask) ** 2).mean()
        losses.append(float(loss.detach()))
        if not loss.requires_grad:
            return losses, params, False
        if step < steps:
            opt.zero_grad(set_to_none=True)
            loss.backward()
            reached = reached and all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in params)
            opt.step()
    return losses, params, reached


def test_a_coverage_mask_loss_moves_the_geometry():
    losses, _, reached = _mask_run(True)
    print(f"mask loss: {losses[0]:.5f} before, {losses[-1]:.5f} after {len(losses) - 1} Adam steps")
    assert len(losses) == 31 and losses[-1] < losses[0]
    assert reached, "every step's gradient reached means3D, scales and opacities"
    off, params_off, _ = _mask_run(False)
    assert len(off) == 1, "with the keyword off the coverage image carries no gradient: the loss cannot be differentiated"
    assert all(p.grad is None for p in params_off), "the geometry leaves receive no gradient at all"
