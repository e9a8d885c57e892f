"""GPU tests of the aux-channel compositing (csrc/render_aux.hip; include/das3r_raster.h das3r_raster_aux_forward / _adjoint): a caller's
[P, C] rows blended over the lists a forward has left behind, the adjoint of that blend, the coverage map read out of the saved image
buffer, and what is built on them (GaussianRasterizer.forward(features=, return_alpha=), das3r_render, render_view_fused, render_set,
psnr_report(static_mask="rendered"), prune.contribution_scores).

References: the float64 dense oracle fed colors_precomp = three feature columns and bg = 0 (the recipe of
tests/test_gpu_invdepth.py::_oracle_invdepth) and its autograd gradient with respect to colors_precomp; the library's own colour path
(forward with colors_precomp = F[:, :3], backward's dL_dcolors_precomp) where the oracle has no form (antialiasing, the `pre` form).
Bars: tests/util.py's, unchanged — the colour path meets them on these very scenes."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

FWD_VARIANTS = ["basic_deg3", "ragged_image", "long_lists", "deep", "culled", "depth_ties", "single"] + util.CAMERA_VARIANTS
ADJ_VARIANTS = ["basic_deg3", "deep", "culled", "long_lists", "frustum_edge"]
PATHS = [("quad", "radix"), ("rows", "local"), ("rows", "seg"), ("lanes", "radix"), ("fine", "radix")]
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


def _forward(rs, kw, dev, colors=None, **more):
    """-> (_forward_full's result, its RasterState); colors: colors_precomp instead of the scene's SH."""
    from das3r_amd import rasterizer
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], e if colors is not None else kw.get("shs", e), colors if colors is not None else e,
                                   kw["opacities"], kw.get("scales", e), kw.get("rotations", e), kw.get("cov3D_precomp", e), **more)
    return res, rasterizer.RasterState.of(res, rs)


def _features(P, width=8, seed=77):
    return torch.rand(P, width, generator=torch.Generator().manual_seed(seed))


def _grad_image(sc, width=3, seed=78):
    """G ~ N(0, 1) / Npix"""
    return torch.randn(width, sc.H, sc.W, generator=torch.Generator().manual_seed(seed)) / float(sc.H * sc.W)


def _dense(kw, skw, colors, bg=None):
    from oracle.dense_oracle import rasterize_dense
    okw = {k: v for k, v in kw.items() if k not in ("shs", "colors_precomp")}
    oskw = {k: v for k, v in skw.items() if k not in ("prefiltered", "debug")}
    oskw["bg"] = torch.zeros(3, dtype=torch.float64, device=colors.device) if bg is None else bg
    m = kw["means3D"]
    return rasterize_dense(means2D=torch.zeros_like(m, dtype=torch.float64), colors_precomp=colors, **okw, **oskw)[0]


_SCENES, _ORACLE_IMG, _ORACLE_ADJ = {}, {}, {}


def _scene(name):
    """(scene, mode, features [P, 8] on the host) — one per variant, shared and never written to"""
    if name not in _SCENES:
        sc, mode = util.scene_variant(name)
        _SCENES[name] = (sc, mode, _features(sc.P))
    return _SCENES[name]


def _oracle_image(name):
    """[8, H, W] float64 (host): the dense oracle's blend of the variant's eight feature columns, three oracle channels at a time, bg = 0.
    Computed once per variant."""
    if name not in _ORACLE_IMG:
        sc, mode, F = _scene(name)
        dev = _dev()
        kw, skw, _ = _inputs(sc, mode, dev)
        Fd = F.to(dev).double()
        with torch.no_grad():
            parts = [_dense(kw, skw, Fd[:, cols].contiguous()) for cols in ([0, 1, 2], [3, 4, 5], [6, 7, 7])]
        _ORACLE_IMG[name] = torch.cat([parts[0], parts[1], parts[2][:2]], 0).cpu()
    return _ORACLE_IMG[name]


def _oracle_adjoint(name):
    """[P, 3] float64 (host): autograd's d<G, image>/d colors_precomp of the dense oracle, G = _grad_image.  Computed once per variant."""
    if name not in _ORACLE_ADJ:
        sc, mode, F = _scene(name)
        dev = _dev()
        kw, skw, _ = _inputs(sc, mode, dev)
        cols = F[:, :3].to(dev).double().clone().requires_grad_(True)
        (_dense(kw, skw, cols) * _grad_image(sc).to(dev).double()).sum().backward()
        _ORACLE_ADJ[name] = cols.grad.cpu()
    return _ORACLE_ADJ[name]


def _check_against_oracle(name, C_, monkeypatch=None, path=None):
    from das3r_amd import _lib, composite_features
    if path is not None:
        monkeypatch.setenv("DAS3R_RENDER", path[0])
        monkeypatch.setenv("DAS3R_BINNING", path[1])
    sc, mode, F = _scene(name)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    _lib.profile_report()
    _lib.profile_enable(True)
    res, state = _forward(rs, kw, dev)
    got = composite_features(state, F[:, :C_].contiguous().to(dev))
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ran = _lib.profile_report()
    assert ran.get("render_aux_forward_kernel", (0,))[0] == 1, ran   # the new kernel, under its stable name; no second forward:
    assert sum(n for k, (n, _) in ran.items() if k.startswith("render_forward")) == 1, ran
    if path is not None:
        assert ran.get(KERNELS[path[0]], (0,))[0] == 1, (path, ran)
    assert got.shape == (C_, sc.H, sc.W) and torch.isfinite(got).all()
    ref = _oracle_image(name)[:C_].numpy()
    got = got.double().cpu().numpy()
    d = np.abs(got - ref)
    print(f"[{name} C={C_} path={path}] max |delta| {d.max():.3e}, fraction over {util.COLOR_TOL}: {(d > util.COLOR_TOL).mean():.2e}")
    util.assert_color_close(got, ref, f"{name} C={C_} {path}")
    assert (got[ref == 0] == 0).all(), "a pixel the oracle leaves empty is exactly 0 (no background term)"


# ------------------------------------------------------------------------------------------------------- 1. forward against the dense oracle
@pytest.mark.parametrize("C_", [1, 3, 4, 8])
@pytest.mark.parametrize("name", FWD_VARIANTS)
def test_forward_against_the_dense_oracle(name, C_):
    """basic_deg3 has a non-zero background: the aux image must carry none."""
    _check_against_oracle(name, C_)


@pytest.mark.parametrize("name", FWD_VARIANTS)
@pytest.mark.parametrize("path", PATHS, ids=["-".join(p) for p in PATHS])
def test_forward_reads_the_lists_of_every_path(name, path, monkeypatch):
    """Every list layout a forward can leave — global sort, local order (sorted in place by the compositing kernel), segmented — and every
    forward kernel's n_contrib."""
    _check_against_oracle(name, 3, monkeypatch, path)


# ------------------------------------------------------------------------------------------------- 2. against the library itself, on every path
def _self_check(sc, mode, F, dev, what, **more):
    """composite_features / feature_adjoint on a forward with colors_precomp = F[:, :3] and bg = 0 against that forward's own colour and
    its backward's dL_dcolors_precomp."""
    from das3r_amd import GaussianRasterizationSettings, composite_features, feature_adjoint, rasterizer
    kw, skw, _ = _inputs(sc, mode, dev)
    rs = GaussianRasterizationSettings(**dict(skw, bg=torch.zeros(3, device=dev)))
    cols = F[:, :3].contiguous().to(dev)
    res, state = _forward(rs, kw, dev, colors=cols, **more)
    img = composite_features(state, cols)
    util.assert_color_close(img.cpu().numpy(), res[1].cpu().numpy(), f"{what}: composite_features vs the forward's own colour")
    G = _grad_image(sc).to(dev)
    e = torch.empty(0, device=dev)
    ref = rasterizer._backward_impl(rs, res[0], G, kw["means3D"], e, cols, kw["opacities"], kw.get("scales", e), kw.get("rotations", e),
                                    kw.get("cov3D_precomp", e), res[3], res[4], res[5], res[6])[1]
    got = feature_adjoint(state, G)
    util.assert_grad_close(got.cpu().numpy(), ref.cpu().numpy(), f"{what}: feature_adjoint vs the backward's dL_dcolors_precomp")
    again = feature_adjoint(state, G)   # ... and after the main backward has run on the same saved state
    assert torch.equal(got, again), what


@pytest.mark.parametrize("name", ["basic_deg3", "long_lists", "deep"])
@pytest.mark.parametrize("path", [None] + PATHS, ids=["default"] + ["-".join(p) for p in PATHS])
def test_against_the_librarys_own_colour_path(name, path, monkeypatch):
    if path is not None:
        monkeypatch.setenv("DAS3R_RENDER", path[0])
        monkeypatch.setenv("DAS3R_BINNING", path[1])
    sc, mode, F = _scene(name)
    _self_check(sc, mode, F, _dev(), f"{name} {path}")


@pytest.mark.parametrize("name", ["basic_deg3", "long_lists"])
def test_antialiased_forward_against_its_own_colour_path(name):
    """The antialiasing factor is folded into the saved opacity: the aux blend of an antialiased forward is antialiased."""
    sc, mode, F = _scene(name)
    _self_check(sc, mode, F, _dev(), f"{name} antialiased", antialiasing=True)


def _loaded_model(seed=3, frames=3, W=64, H=48):
    """A model as offline.load_trained_model hands it over (plain tensors, one conf_static value per Gaussian, full SH degree), its cameras
    and poses — from a small synthetic sequence; the confidences are random so that the static map is not a constant."""
    from das3r_amd.model import SplatModel
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    seq = synthetic_sequence(frames=frames, W=W, H=H, focal=70.0, n_splats=1500, seed=seed)
    src, cams = build_from_sequence(seq, sh_degree=1)
    m = SplatModel(1)
    for n in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        setattr(m, n, getattr(src, n).detach().clone().contiguous())
    P = m._xyz.shape[0]
    m._conf_static = (0.2 + 0.8 * torch.rand(P, 1, generator=torch.Generator().manual_seed(seed))).cuda()
    m.active_sh_degree = 1
    for c in cams:
        c.pose7 = src.get_RT(c.uid).detach().clone()
    return m, cams


def test_pre_form_through_render_view_fused():
    """The forward with the pose pre-transform inside its kernels (das3r_raster_in.pre): its aux image against the glue form's colour render of
    the same columns (override_color, bg = 0), its adjoint against that render's backward."""
    from das3r_amd import feature_adjoint, offline
    from das3r_amd.render import das3r_render
    dev = _dev()
    model, cams = _loaded_model()
    P = model._xyz.shape[0]
    F = _features(P, 3).to(dev)
    bg = torch.zeros(3, device=dev)
    view = cams[1]
    img, radii, fimg, alpha, state = offline.render_view_fused(model, view, view.pose7, bg, features=F, alpha=True, return_state=True)
    assert fimg.shape == (3, view.image_height, view.image_width) and alpha.shape == (1, view.image_height, view.image_width)
    cols = F.clone().requires_grad_(True)
    with torch.enable_grad():
        glue = das3r_render(view, model, offline.PIPE, bg, camera_pose=view.pose7, variant="test", override_color=cols)["render"]
        G = torch.randn(glue.shape, generator=torch.Generator().manual_seed(5)).to(dev) / float(glue[0].numel())
        (glue * G).sum().backward()
    util.assert_color_close(fimg.cpu().numpy(), glue.detach().cpu().numpy(), "pre form: aux image vs the glue form's colour render")
    util.assert_grad_close(feature_adjoint(state, G).cpu().numpy(), cols.grad.cpu().numpy(), "pre form: adjoint vs the glue form's backward")
    # and the maps render_set hands out: the model's own conf_static column, the coverage
    smaps, amaps = [], []
    imgs = offline.render_set("unused", "interp", 0, cams[:2], model, background=bg, write=False, fused=True, static_map=smaps, alpha=amaps)
    glue_s, glue_a = [], []
    offline.render_set("unused", "interp", 0, cams[:2], model, background=bg, write=False, fused=False, static_map=glue_s, alpha=glue_a)
    assert len(imgs) == len(smaps) == len(amaps) == 2
    for a, b, x, y in zip(smaps, glue_s, amaps, glue_a):
        assert a.shape == x.shape == (1, view.image_height, view.image_width)
        util.assert_color_close(a.cpu().numpy(), b.cpu().numpy(), "static map: fused vs glue")
        util.assert_color_close(x.cpu().numpy(), y.cpu().numpy(), "alpha map: fused vs glue")
        assert float(a.max()) <= 1.0 + 1e-5 and float(a.min()) >= 0.0 and float((a <= x + 1e-5).float().mean()) == 1.0   # conf <= 1: static <= alpha


def test_render_set_writes_the_maps(tmp_path):
    from das3r_amd import offline
    model, cams = _loaded_model(W=48, H=32)
    smaps, amaps, inv = [], [], []
    offline.render_set(str(tmp_path), "interp", 7, cams[:1], model, write=True, fused=True, invdepth=inv, static_map=smaps, alpha=amaps)
    base = tmp_path / "interp" / "ours_7"
    for sub, ref in (("static", smaps[0]), ("alpha", amaps[0]), ("invdepth", inv[0])):
        arr = np.load(base / sub / "00000.npy")
        assert arr.shape == (32, 48) and arr.dtype == np.float32 and np.array_equal(arr, ref[0].cpu().numpy()), sub


# ----------------------------------------------------------------------------------------------------------------------------------- 3. alpha
@pytest.mark.parametrize("name", ["basic_deg3", "long_lists", "deep", "culled", "ragged_image"])
def test_alpha_is_the_blend_of_ones_and_zero_where_nothing_was_blended(name):
    from das3r_amd import _lib, alpha_of, composite_features
    sc, mode, _ = _scene(name)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    res, state = _forward(rs, kw, dev, exact=True)
    _lib.profile_report()
    _lib.profile_enable(True)
    alpha = alpha_of(state)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    assert _lib.profile_report() == {}, "alpha_of launches no kernel of the library"
    assert alpha.shape == (1, sc.H, sc.W) and float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0
    ones = composite_features(state, torch.ones(sc.P, 1, device=dev))
    util.assert_color_close(ones.cpu().numpy(), alpha.cpu().numpy(), f"{name}: blend of ones vs 1 - final_T")
    L = _lib.layout(sc.P, res[0], sc.W, sc.H)
    n_contrib = res[5][L["n_contrib"]:L["n_contrib"] + 4 * sc.W * sc.H].view(torch.int32).reshape(1, sc.H, sc.W)
    assert (alpha[n_contrib == 0] == 0).all() and (ones[n_contrib == 0] == 0).all()


# --------------------------------------------------------------------------------------------------- 4. adjoint against the oracle's autograd
@pytest.mark.parametrize("name", ADJ_VARIANTS)
def test_adjoint_against_the_dense_oracles_gradient(name):
    from das3r_amd import _lib, feature_adjoint
    sc, mode, _ = _scene(name)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    _, state = _forward(rs, kw, dev)
    _lib.profile_report()
    _lib.profile_enable(True)
    got = feature_adjoint(state, _grad_image(sc).to(dev))
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ran = _lib.profile_report()
    assert ran.get("render_aux_adjoint_kernel", (0,))[0] == 1 and ran.get("aux_gather_kernel", (0,))[0] == 1 and len(ran) == 2, ran
    ref = _oracle_adjoint(name).numpy()
    rel = np.abs(got.double().cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"[{name}] adjoint: max |delta| / max |ref| = {rel:.3e} (bar {util.GRAD_REL_TOL})")
    util.assert_grad_close(got.cpu().numpy(), ref, f"{name}: adjoint vs autograd of the dense oracle")


@pytest.mark.parametrize("width", [1, 2, 8, 11])
def test_adjoint_of_every_width_matches_the_three_channel_one(width):
    """The reduction differs by width (one value: a DPP chain; more: the transposed reduction; more than 8: several calls) — channel c of
    any width is the same sum."""
    from das3r_amd import feature_adjoint
    sc, mode, _ = _scene("ragged_image")
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    _, state = _forward(rs, kw, dev)
    G = _grad_image(sc, 11, seed=9).to(dev)
    ref = torch.cat([feature_adjoint(state, G[c0:c0 + 3].contiguous()) for c0 in (0, 3, 6, 9)], 1)[:, :11]
    # (the three-channel adjoint itself is held to the oracle above)
    got = feature_adjoint(state, G[:width].contiguous())
    util.assert_grad_close(got.cpu().numpy(), ref[:, :width].cpu().numpy(), f"width {width}")


# ------------------------------------------------------------------------------------------------------ 5. fully written and reproducible
def _raw_adjoint(state, G, out, accumulate, scratch):
    from das3r_amd import _lib
    from das3r_amd.rasterizer import _stream
    a, saved = state._c_args()
    rc = _lib.load().das3r_raster_aux_adjoint(C.byref(a), C.byref(saved), G.shape[0], C.c_void_p(G.data_ptr()), C.c_void_p(out.data_ptr()),
                                              int(accumulate), C.c_void_p(scratch.data_ptr()), _stream(state.device))
    _lib.check(rc, "das3r_raster_aux_adjoint")
    return out


@pytest.mark.parametrize("C_", [1, 3, 8])
@pytest.mark.parametrize("name", ["culled", "long_lists", "basic_deg3", "deep"])
def test_adjoint_is_fully_written_and_reproducible(name, C_):
    from das3r_amd import _lib
    sc, mode, _ = _scene(name)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    res, state = _forward(rs, kw, dev)
    G = _grad_image(sc, C_, seed=4).to(dev)
    nbytes = _lib.load().das3r_raster_aux_scratch_bytes(int(state.capacity), C_)
    runs = []
    for _ in range(2):
        scratch = torch.full(((nbytes + 3) // 4,), float("nan"), device=dev)
        out = torch.full((sc.P, C_), float("nan"), device=dev)
        _lib.poison_lds(0x7FC00000)
        runs.append(_raw_adjoint(state, G, out, False, scratch))
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0]).all(), "every row is written, from sums that read nothing unwritten"
    assert torch.equal(runs[0], runs[1]), "bit-identical from run to run"
    unrendered = res[2] == 0
    assert unrendered.any() or name != "culled"
    assert (runs[0][unrendered] == 0).all(), "a Gaussian without instances gets an exact zero row"
    assert float(runs[0].abs().max()) > 0
    acc = torch.zeros(sc.P, C_, device=dev)
    scratch = torch.full(((nbytes + 3) // 4,), float("nan"), device=dev)
    _raw_adjoint(state, G, acc, True, scratch)
    _raw_adjoint(state, G, acc, True, scratch)
    assert torch.equal(acc, 2.0 * runs[0]), "one writer per element: accumulating twice is exactly twice the sum"


@pytest.mark.parametrize("name,split", [("basic_deg3", False), ("culled", False), ("long_lists", True), ("deep", True)])
def test_few_tiles_with_long_lists_take_the_split_forward(name, split):
    """The threshold between the two forms of the kernels (render_aux.hip aux_long_lists: at most 1024 tiles, 1024 or more entries per tile on
    average): `long_lists` (12 tiles of ~1400 entries) and `deep` (6 tiles of ~4000: several buckets each) are beyond it and take the forward
    with four workgroups per tile and the bucket-parallel adjoint, the others one workgroup per tile.  Both forms are held to the oracle
    above."""
    from das3r_amd import _lib, composite_features
    sc, mode, F = _scene(name)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    res, state = _forward(rs, kw, dev)
    ntiles = ((sc.W + 15) // 16) * ((sc.H + 15) // 16)
    assert (res[0] >= 1024 * ntiles) == split, (res[0], ntiles)
    if name == "deep":
        assert res[0] > 2 * 1024 * ntiles, "more than one bucket per tile: the adjoint's workgroups start from the forward's checkpoints"
    _lib.profile_report()
    _lib.profile_enable(True)
    composite_features(state, F[:, :3].contiguous().to(dev))
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    ran = _lib.profile_report(raw=True)
    assert list(ran) == ["render_aux_forward_kernel<CC, true>" if split else "render_aux_forward_kernel<CC, false>"], ran


@pytest.mark.parametrize("name", ["long_lists", "deep"])
def test_forward_reads_nothing_it_has_not_written(name):
    from das3r_amd import _lib, composite_features
    sc, mode, F = _scene(name)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    _, state = _forward(rs, kw, dev)
    f = F.to(dev)
    a = composite_features(state, f)
    _lib.poison_lds(0x7FC00000)
    b = composite_features(state, f)
    assert torch.isfinite(b).all() and torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------------- 6. nothing else moves
def _run_rasterizer(sc, mode, dev, features=None, return_alpha=False):
    from das3r_amd import GaussianRasterizer
    kw = {k: v.to(dev).clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
    _, _, rs = _inputs(sc, mode, dev)
    kw["means2D"] = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    extra = {}
    if features is not None:
        extra["features"] = features
    if return_alpha:
        extra["return_alpha"] = True
    return GaussianRasterizer(rs)(**kw, **extra), kw


@pytest.mark.parametrize("name", ["basic_deg3", "culled"])
def test_colour_radii_and_colour_gradients_do_not_move(name, monkeypatch):
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")   # (the pixel-per-lane backward meets its waves with LDS atomics: bit-equality needs the fixed order)
    sc, mode, F = _scene(name)
    dev = _dev()
    dL = sc.dL_dpix.to(dev)
    out0, kw0 = _run_rasterizer(sc, mode, dev)
    assert len(out0) == 2
    (out0[0] * dL).sum().backward()
    feats = F[:, :4].contiguous().to(dev).requires_grad_(True)
    out1, kw1 = _run_rasterizer(sc, mode, dev, features=feats, return_alpha=True)
    assert len(out1) == 4 and out1[2].shape == (4, sc.H, sc.W) and out1[3].shape == (1, sc.H, sc.W)
    (out1[0] * dL).sum().backward()
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1])
    for k in kw0:
        assert torch.equal(kw0[k].grad, kw1[k].grad), k
    assert feats.grad is None, "a colour loss sends nothing to the features"
    out2, _ = _run_rasterizer(sc, mode, dev, return_alpha=True)
    assert len(out2) == 3 and torch.equal(out2[2], out1[3]) and torch.equal(out2[0], out0[0])


@pytest.mark.parametrize("order", ["colour_first", "features_first"])
def test_a_feature_loss_reaches_the_features_alone_in_either_order(order, monkeypatch):
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    name = "basic_deg3"
    sc, mode, F = _scene(name)
    dev = _dev()
    dL, G = sc.dL_dpix.to(dev), _grad_image(sc).to(dev)
    # the colour gradients of a run without features
    out0, kw0 = _run_rasterizer(sc, mode, dev)
    (out0[0] * dL).sum().backward()
    feats = F[:, :3].contiguous().to(dev).requires_grad_(True)
    out, kw = _run_rasterizer(sc, mode, dev, features=feats)
    colour_loss, feature_loss = (out[0] * dL).sum(), (out[2] * G).sum()
    first, second = (colour_loss, feature_loss) if order == "colour_first" else (feature_loss, colour_loss)
    first.backward(retain_graph=True)
    if order == "features_first":   # a loss on the feature image alone: geometry, SH and opacity get nothing
        for k, v in kw.items():
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
    second.backward()
    util.assert_grad_close(feats.grad.cpu().numpy(), _oracle_adjoint(name).numpy(), f"features.grad, {order}")
    for k in kw0:
        assert torch.equal(kw0[k].grad, kw[k].grad), (order, k)


# ------------------------------------------------------------------------------------------------------------------------- 7. edge shapes
def test_empty_scene():
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer, feature_adjoint
    sc, mode, _ = _scene("single")
    dev = _dev()
    _, skw, rs = _inputs(sc, mode, dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    r = GaussianRasterizer(rs)
    color, radii, fimg, alpha = r(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4),
                                  features=z(0, 5), return_alpha=True)
    assert fimg.shape == (5, sc.H, sc.W) and alpha.shape == (1, sc.H, sc.W) and radii.numel() == 0
    assert float(fimg.abs().max()) == 0.0 and float(alpha.abs().max()) == 0.0
    g = feature_adjoint(r.state, torch.ones(5, sc.H, sc.W, device=dev))
    assert g.shape == (0, 5)


def test_image_smaller_than_a_tile():
    from das3r_amd import alpha_of, composite_features, feature_adjoint
    from das3r_amd.synth import make_scene
    sc = make_scene(P=40, W=7, H=5, focal=6.0, sh_degree=0, seed=41, s_px=(0.8, 2.5))
    mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    F = _features(sc.P, 3, seed=42)
    _, state = _forward(rs, kw, dev)
    img = composite_features(state, F.to(dev))
    with torch.no_grad():
        ref = _dense(kw, skw, F.to(dev).double())
    assert float(ref.abs().max()) > 0
    util.assert_color_close(img.cpu().numpy(), ref.cpu().numpy(), "7x5 image")
    cols = F.to(dev).double().requires_grad_(True)
    G = _grad_image(sc, seed=43)
    (_dense(kw, skw, cols) * G.to(dev).double()).sum().backward()
    util.assert_grad_close(feature_adjoint(state, G.to(dev)).cpu().numpy(), cols.grad.cpu().numpy(), "7x5 adjoint")
    assert alpha_of(state).shape == (1, 5, 7)


def test_eight_channels_on_a_ragged_image_both_ways():
    """C = 8 forward on ragged_image is in test 1; here its adjoint, against the backward's dL_dcolors_precomp three channels at a time."""
    from das3r_amd import GaussianRasterizationSettings, feature_adjoint, rasterizer
    sc, mode, F = _scene("ragged_image")
    dev = _dev()
    kw, skw, _ = _inputs(sc, mode, dev)
    rs = GaussianRasterizationSettings(**dict(skw, bg=torch.zeros(3, device=dev)))
    cols = F[:, :3].contiguous().to(dev)
    res, state = _forward(rs, kw, dev, colors=cols)
    G = _grad_image(sc, 8, seed=12).to(dev)
    got = feature_adjoint(state, G)
    e = torch.empty(0, device=dev)
    for c0 in (0, 3, 5):
        ref = rasterizer._backward_impl(rs, res[0], G[c0:c0 + 3].contiguous(), kw["means3D"], e, cols, kw["opacities"], kw["scales"], kw["rotations"], e,
                                        res[3], res[4], res[5], res[6])[1]
        util.assert_grad_close(got[:, c0:c0 + 3].cpu().numpy(), ref.cpu().numpy(), f"C = 8 adjoint, channels {c0}..{c0 + 2}")


def test_wide_features_are_split_into_calls_of_eight():
    from das3r_amd import composite_features
    sc, mode, _ = _scene("basic_deg3")
    dev = _dev()
    kw, skw, rs = _inputs(sc, mode, dev)
    _, state = _forward(rs, kw, dev)
    F = _features(sc.P, 19, seed=6).to(dev).requires_grad_(True)
    img = composite_features(state, F)
    assert img.shape == (19, sc.H, sc.W)
    for c0 in (0, 8, 16):
        assert torch.equal(img[c0:c0 + 8].detach(), composite_features(state, F.detach()[:, c0:c0 + 8].contiguous()))
    G = _grad_image(sc, 19, seed=7).to(dev)
    (img * G).sum().backward()
    from das3r_amd import feature_adjoint
    assert torch.equal(F.grad[:, 8:16], feature_adjoint(state, G[8:16].contiguous()))


# ------------------------------------------------------------------------------------------------------------------ 8. contribution scores
def test_contribution_scores_sum_the_blending_weights_over_views():
    from das3r_amd.prune import contribution_scores, prune_points
    from das3r_amd.render import rasterizer_inputs
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    from oracle.dense_oracle import rasterize_dense
    from types import SimpleNamespace
    dev = _dev()
    seq = synthetic_sequence(frames=3, W=48, H=32, focal=44.0, n_splats=1500, seed=8)
    model, cams = build_from_sequence(seq, sh_degree=0)
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device=dev)
    scores = contribution_scores(model, cams, pipe, bg)
    P = model._xyz.shape[0]
    assert scores.shape == (P,) and scores.dtype == torch.float32
    assert torch.equal(scores, contribution_scores(model, cams, pipe, bg)), "bit-identical from run to run"
    ref = torch.zeros(P, dtype=torch.float64, device=dev)
    for cam in cams:
        with torch.no_grad():
            settings, kw = rasterizer_inputs(cam, model, pipe, bg, camera_pose=model.get_RT(cam.uid))
        okw = {k: v.detach() for k, v in kw.items() if v is not None and k not in ("shs", "colors_precomp", "means2D")}
        skw = {k: v for k, v in settings._asdict().items() if k not in ("prefiltered", "debug")}
        cols = torch.zeros(P, 3, dtype=torch.float64, device=dev, requires_grad=True)
        img = rasterize_dense(means2D=torch.zeros(P, 3, dtype=torch.float64, device=dev), colors_precomp=cols, **okw, **skw)[0]
        img[0].sum().backward()   # a ones image on one channel
        ref += cols.grad[:, 0]
    assert float(ref.max()) > 0.0
    util.assert_grad_close(scores.cpu().numpy(), ref.cpu().numpy(), "contribution_scores vs the summed oracle gradients of a ones image")
    # the hand-off: the Gaussians that make up least of the views go
    tau = float(scores.median())
    gone = int((scores < tau).sum())
    assert 0 < gone < P
    info = prune_points(model, min_opacity=0.0, also_drop=scores < tau)
    assert info["dropped"] == gone and model._xyz.shape[0] == P - gone


# ------------------------------------------------------------------------------------------------------ 9. the report's rendered static mask
def test_psnr_report_with_the_rendered_static_mask():
    from das3r_amd import _lib
    from das3r_amd.losses import l1_loss, psnr
    from das3r_amd.prune import mask_index
    from das3r_amd.render import das3r_render
    from das3r_amd.train import build_from_sequence, consistent_sequence, psnr_report, resize_mask_nearest
    from types import SimpleNamespace
    dev = _dev()
    seq = consistent_sequence(frames=16, W=96, H=64, focal=110.0, n_splats=3000, seed=2)
    model, cams, test = build_from_sequence(seq, sh_degree=0, heldout=True)
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    bg = torch.zeros(3, device=dev)
    masks = {c.uid: torch.from_numpy(seq["gt_dynamic_masks"][c.frame_index]) for c in test}
    conf = model._conf_static.detach().reshape(-1)[mask_index(model)].reshape(-1, 1).float().contiguous()
    maps = {}

    def by_hand(view):
        """the report's arithmetic, restated: view(camera) -> (render, static mask)"""
        _lib.forget_shapes()   # (every pass starts from the library state a fresh thread finds: the same kernels, view for view)
        l1s, ps = 0.0, 0.0
        for c in test:
            with torch.no_grad():
                img, s = view(c)
            img, gt = img.clamp(0, 1), c.original_image.clamp(0, 1)
            l1s += float(l1_loss(img * s, gt * s).mean().double())
            ps += float(psnr(img * s, gt * s).mean().double())
        return l1s / len(test), ps / len(test)

    def report(**kw):
        _lib.forget_shapes()
        return psnr_report(model, test, test_poses=True, **kw)

    def close(rep, want):
        return abs(rep["psnr"] - want[1]) < 1e-4 and abs(rep["l1"] - want[0]) < 1e-5 * abs(want[0])

    # "gt": the report as it was, value for value (and the default)
    want = by_hand(lambda c: (das3r_render(c, model, pipe, bg, camera_pose=model.get_RT_test(c.uid))["render"],
                              1 - resize_mask_nearest(masks[c.uid].to(dev), 64, 96)))
    rep, rep_gt = report(dynamic_masks=masks), report(dynamic_masks=masks, static_mask="gt")
    assert rep == rep_gt and rep["views"] == len(test) == 2
    assert close(rep, want), (rep, want)

    # "rendered": masked with the model's own static map at the held-out pose, from the same forward as the image
    def rendered(c, thr=0.5):
        pkg = das3r_render(c, model, pipe, bg, camera_pose=model.get_RT_test(c.uid), features=conf)
        maps[c.uid] = pkg["features"]
        return pkg["render"], (pkg["features"] >= thr).float()

    want_r = by_hand(rendered)
    rep_r = report(dynamic_masks=None, static_mask="rendered")
    assert rep_r["views"] == 2 and rep_r["skipped"] == 0
    assert close(rep_r, want_r), (rep_r, want_r)
    assert all(m.shape == (1, 64, 96) for m in maps.values())
    frac = float(torch.cat([(m >= 0.5).float().reshape(-1) for m in maps.values()]).mean())
    print(f"the rendered static mask keeps {frac:.3f} of the held-out pixels; PSNR gt-masked {rep['psnr']:.3f}, rendered-masked {rep_r['psnr']:.3f}")
    assert 0.05 < frac < 1.0, f"the rendered mask keeps {frac:.2f} of the pixels: neither everything nor nothing"
    assert rep_r["psnr"] != rep["psnr"]
    strict = report(static_mask="rendered", static_threshold=0.9)
    assert close(strict, by_hand(lambda c: rendered(c, 0.9)))
