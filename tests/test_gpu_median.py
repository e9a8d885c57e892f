"""GPU tests of the median depth and the surface hit (csrc/render_median.hip; include/das3r_raster.h das3r_raster_median_forward /
das3r_raster_median_adjoint) and of what is built on them: das3r_amd.median_depth_of(state, geometry=), median_hit_adjoint,
das3r_render(return_median_depth=), prune.surface_scores.

Reference: tests/median_reference.py — the float64 dense oracle's weights, the hit taken from their running transmittance.  The hit is a
selection, so the comparison is a bracket: with delta = util.COLOR_TOL * tau (the project's bar on blended quantities in [0, 1], relative to
tau) the library's hit must be an entry the reference could have picked with a T off by at most delta — T_before > tau - delta, and the last
contributor or T_after <= tau + delta — on EVERY covered pixel; on the pixels the reference is at least delta away from another choice
(tests/test_median_reference_host.py: at least 95 % of them) it must be the reference's own hit, with its depth to util.GRAD_REL_TOL of the
largest.  Bars: tests/util.py's, unchanged."""
import copy
from types import SimpleNamespace

import pytest
import torch

from tests import median_reference as mref
from tests import util
from tests.test_gpu_distortion import PATHS, _dev, _inputs, _raw, _render, _scene

pytestmark = pytest.mark.gpu

VARIANTS = ["basic_deg3", "ragged_image", "long_lists", "deep", "culled", "depth_ties", "cov3D_precomp", "single"] + util.CAMERA_VARIANTS
PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
EMPTY = -1   # the u32 position plane's 0xFFFFFFFF in the int32 tensor that holds it, and the Gaussian plane's -1

_REF = {}


def _reference(name, tau=0.5, antialiased=False):
    """median_reference of the variant on the device, computed once per (variant, tau, antialiased) and never written to"""
    key = (name, tau, antialiased)
    if key not in _REF:
        sc, mode, _ = _scene(name)
        _REF[key] = mref.reference_of_scene(sc, mode, tau, _dev(), antialiased)
    return _REF[key]


def _n_contrib(state):
    from das3r_amd import _lib
    L = _lib.layout(state.P, int(state.capacity) if int(state.capacity) > 0 else state.num_rendered, state.W, state.H)
    return state.img[L["n_contrib"]:L["n_contrib"] + 4 * state.H * state.W].view(torch.int32).reshape(state.H, state.W)


def _planes(state, tau=0.5):
    from das3r_amd import median_depth_of
    depth, hit_g, hit_p = median_depth_of(state, threshold=tau, return_hit=True, return_position=True)
    assert depth.shape == (1, state.H, state.W) and depth.dtype == torch.float32 and not depth.requires_grad
    assert hit_g.shape == hit_p.shape == (state.H, state.W) and hit_g.dtype == hit_p.dtype == torch.int32
    return depth[0], hit_g, hit_p


def _hold_to_reference(state, r, tau, what):
    """The module docstring's comparison -> the three planes."""
    depth, hit_g, hit_p = _planes(state, tau)
    delta = util.COLOR_TOL * tau
    empty = (_n_contrib(state) == 0).reshape(-1)
    d, g, p = depth.reshape(-1), hit_g.reshape(-1).long(), hit_p.reshape(-1).long()
    # empty pixels: exactly 0 / -1 / 0xFFFFFFFF; every other pixel has a hit
    assert bool((d[empty] == 0).all()) and bool((g[empty] == EMPTY).all()) and bool((p[empty] == EMPTY).all())
    assert bool((g[~empty] >= 0).all()) and bool((g[~empty] < state.P).all()) and bool((p[~empty] >= 0).all())
    covered = r["covered"]
    assert torch.equal(covered, ~empty), f"{what}: the library and the reference disagree on which pixels are covered"
    # the library's hit in the reference's columns
    col_of = torch.empty_like(r["order"])
    col_of[r["order"]] = torch.arange(r["order"].numel(), device=col_of.device)
    col = col_of[g.clamp(min=0)][:, None]
    kept = r["keep"].gather(1, col)[:, 0]
    Tb, Ta = r["T_before"].gather(1, col)[:, 0], r["T_after"].gather(1, col)[:, 0]
    last = col[:, 0] == r["last_col"]
    ok = kept & (Tb > tau - delta) & (last | (Ta <= tau + delta))
    bad = covered & ~ok
    exact = covered & (r["margin"] >= delta)
    share = float(exact.sum()) / max(float(covered.sum()), 1.0)
    same = g == r["hit_gaussian"]
    zmax = float(r["depth"].max())
    zerr = float((d.double() - r["depth"])[exact].abs().max()) if bool(exact.any()) else 0.0
    excursion = torch.maximum((tau - Tb).clamp(min=0), torch.where(last, torch.zeros_like(Ta), (Ta - tau).clamp(min=0)))
    worst = float(excursion[covered & kept].max()) if bool((covered & kept).any()) else 0.0
    print(f"[{what}] covered {int(covered.sum())}, outside the bracket {int(bad.sum())} (worst excursion of the reference's T at the library's hit "
          f"{worst:.3e}, delta {delta:.1e}), margin >= delta on {100 * share:.2f} %, of those {int((exact & ~same).sum())} differ, "
          f"max |depth - z_ref| / max z_ref = {zerr / zmax:.3e} (bar {util.GRAD_REL_TOL})")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} covered pixels hit an entry outside the bracket"
    assert share >= 0.95
    assert bool(same[exact].all()), f"{what}: {int((exact & ~same).sum())} pixels away from any other choice do not hit the reference's Gaussian"
    assert zerr <= util.GRAD_REL_TOL * zmax
    return depth, hit_g, hit_p


# ------------------------------------------------------------------------------------------------ 1. forward against the float64 reference
@pytest.mark.parametrize("name", VARIANTS)
def test_forward_against_the_reference(name):
    dev = _dev()
    with torch.no_grad():
        _, _, state, _ = _render(name, dev)
        depth, hit_g, _ = _hold_to_reference(state, _reference(name), 0.5, name)
    assert torch.isfinite(depth).all()
    if name == "single":
        assert bool((hit_g[_n_contrib(state) > 0] == 0).all()) and bool((_n_contrib(state) > 0).any()), "one Gaussian: every covered pixel hits it"


# ------------------------------------------------------------------------------------------------ 2. the hit past one staged batch
def test_a_low_threshold_on_the_deep_scene_hits_past_one_staged_batch():
    dev = _dev()
    with torch.no_grad():
        _, _, state, _ = _render("deep", dev)
        _, _, hit_p = _planes(state, 0.05)
        assert int(hit_p.max()) >= 256, "the hit lies past the first batch of 256 staged entries"
        _hold_to_reference(state, _reference("deep", 0.05), 0.05, "deep tau=0.05")


# ------------------------------------------------------------------------------------------- 3. every forward kernel and binning path
@pytest.mark.parametrize("name", ["basic_deg3", "long_lists"])
@pytest.mark.parametrize("path", PATHS, ids=["-".join(p) for p in PATHS])
def test_forced_kernel_and_binning_pairs(name, path, monkeypatch):
    """The lists differ in provenance, the result must not — within the same bracket."""
    monkeypatch.setenv("DAS3R_RENDER", path[0])
    monkeypatch.setenv("DAS3R_BINNING", path[1])
    _, state, _, _ = _raw(name, _dev())
    _hold_to_reference(state, _reference(name), 0.5, f"{name} {path}")


def test_antialiased_forward_against_the_reference_with_the_factor():
    """The saved opacity carries the factor: no special case."""
    name = "basic_deg3"
    _, state, _, _ = _raw(name, _dev(), antialiasing=True)
    _hold_to_reference(state, _reference(name, antialiased=True), 0.5, f"{name} antialiased")


@pytest.mark.parametrize("name", ["basic_deg3", "deep"])
def test_forward_with_invdepth_leaves_the_same_planes(name):
    dev = _dev()
    plain = _planes(_raw(name, dev)[1])
    with_depth = _planes(_raw(name, dev, invdepth=True)[1])
    for a, b in zip(plain, with_depth):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------------------- 4. crisp cases
@pytest.mark.parametrize("front,expected", [(0.3, 1), (0.6, 0)])
def test_two_gaussians_on_the_centre_pixel(front, expected):
    """T_1 = 1 - front opacity at the pixel both are centred on: 0.7 > 1/2 hits the back one, 0.4 <= 1/2 the front one."""
    from das3r_amd import rasterizer
    from das3r_amd.synth import make_scene
    W, H = 65, 33   # odd: the optical axis meets the centre of pixel (32, 16); wide enough for pixels neither Gaussian reaches
    sc = make_scene(P=2, W=W, H=H, focal=30.0, sh_degree=0, seed=1, s_px=(1.0, 1.0))
    sc.means3D[:] = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 4.0]])
    sc.opacities[:] = torch.tensor([[front], [0.4]])
    mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
    dev = _dev()
    kw, _, rs = _inputs(sc, mode, dev)
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    state = rasterizer.RasterState.of(res, rs)
    assert (res[2] > 0).all(), "both are rendered"
    depth, hit_g, hit_p = _planes(state)
    assert int(hit_g[16, 32]) == expected and int(hit_p[16, 32]) == expected
    assert float(depth[16, 32]) > 0
    empty = _n_contrib(state) == 0
    assert bool(empty.any()) and bool((~empty).any())
    assert bool((depth[empty] == 0).all()) and bool((hit_g[empty] == EMPTY).all()) and bool((hit_p[empty] == EMPTY).all())
    assert bool((hit_g[~empty] >= 0).all()) and bool((depth[~empty] > 0).all())
    _hold_to_reference(state, mref.reference_of_scene(sc, mode, 0.5, dev), 0.5, f"two Gaussians, front opacity {front}")


def test_image_smaller_than_a_tile():
    from das3r_amd import rasterizer
    from das3r_amd.synth import make_scene
    sc = make_scene(P=40, W=8, H=8, focal=7.0, sh_degree=0, seed=41, s_px=(0.8, 2.5))
    mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
    dev = _dev()
    kw, _, rs = _inputs(sc, mode, dev)
    e = torch.empty(0, device=dev)
    res = rasterizer._forward_full(rs, kw["means3D"], kw["shs"], e, kw["opacities"], kw["scales"], kw["rotations"], e)
    state = rasterizer.RasterState.of(res, rs)
    for tau in (0.5, 0.1):
        _hold_to_reference(state, mref.reference_of_scene(sc, mode, tau, dev), tau, f"8x8 image tau={tau}")


def test_empty_scene():
    from das3r_amd import AuxGeometry, GaussianRasterizer, median_depth_of, median_hit_adjoint
    sc, mode = _scene("single")[:2]
    dev = _dev()
    _, _, rs = _inputs(sc, mode, dev)
    z = lambda *s: torch.zeros(*s, device=dev, requires_grad=True)
    kw = dict(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), colors_precomp=z(0, 3), scales=z(0, 3), rotations=z(0, 4))
    r = GaussianRasterizer(rs, keep_state=True)
    r(**kw)
    depth, hit_g, hit_p = median_depth_of(r.state, return_hit=True, return_position=True)
    assert depth.shape == (1, sc.H, sc.W) and float(depth.abs().max()) == 0.0
    assert bool((hit_g == EMPTY).all()) and bool((hit_p == EMPTY).all())
    assert median_hit_adjoint(r.state, torch.ones(sc.H, sc.W, device=dev), hit_p).shape == (0,)
    D = median_depth_of(r.state, geometry=AuxGeometry(rs, **kw))
    assert D.shape == (1, sc.H, sc.W) and float(D.detach().abs().max()) == 0.0
    D.sum().backward()
    assert kw["means3D"].grad is not None and kw["means3D"].grad.shape == (0, 3)


@pytest.mark.parametrize("name", ["basic_deg3", "deep"])
def test_depth_does_not_increase_with_the_threshold(name):
    dev = _dev()
    with torch.no_grad():
        _, _, state, _ = _render(name, dev)
        a, b, c = (_planes(state, tau) for tau in (0.25, 0.5, 0.75))
    assert bool((a[0] >= b[0]).all()) and bool((b[0] >= c[0]).all()), "depth is non-increasing in the threshold at every pixel, exactly"
    assert bool((a[2] >= b[2]).all()) and bool((b[2] >= c[2]).all()) and bool((a[2] > c[2]).any())


# ------------------------------------------------------------------------------------------------------------------------------ 5. adjoint
@pytest.mark.parametrize("name", ["basic_deg3", "ragged_image", "long_lists", "deep", "culled"])
def test_adjoint(name):
    from das3r_amd import _lib, median_hit_adjoint
    dev = _dev()
    G = _scene(name)[2].to(dev)[0].contiguous()
    tau = 0.05 if name == "deep" else 0.5   # (deep: the hits past one staged batch)
    _, state, _, _ = _raw(name, dev)
    _, hit_g, hit_p = _planes(state, tau)
    covered = hit_g >= 0
    nan = float("nan")
    _lib.poison_lds(0x7FC00000)
    dz = median_hit_adjoint(state, G, hit_p, _fill=nan)   # output and scratch pre-filled with NaN
    assert dz.shape == (state.P,) and torch.isfinite(dz).all(), "fully written, from sums that read nothing unwritten"
    # against a float64 index_add of g over the library's own hit plane
    ref = torch.zeros(state.P, dtype=torch.float64, device=dev).index_add_(0, hit_g[covered].long(), G[covered].double())
    print(f"[{name}] dL_dz: max |delta| / max |ref| = {float((dz.double() - ref).abs().max() / ref.abs().max()):.3e} (bar {util.GRAD_REL_TOL})")
    util.assert_grad_close(dz.cpu().numpy(), ref.cpu().numpy(), f"{name}: dL_dz")
    assert bool((dz[ref == 0] == 0).all()), "a Gaussian that is nobody's hit gets an exact zero"
    # two runs are bit-identical
    _lib.poison_lds(0x7FC00000)
    assert torch.equal(dz, median_hit_adjoint(state, G, hit_p, _fill=nan))
    # g = 1: the per-Gaussian pixel count, exactly
    ones = torch.ones_like(G)
    count = median_hit_adjoint(state, ones, hit_p)
    assert torch.equal(count, torch.bincount(hit_g[covered].long(), minlength=state.P).float())
    assert float(count.double().sum()) == float(covered.sum()) and float(covered.sum()) > 0
    # accumulate adds
    acc = count.clone()
    median_hit_adjoint(state, ones, hit_p, out=acc, accumulate=True)
    assert torch.equal(acc, 2.0 * count)
    # no hit anywhere: zeros, and nothing indexed outside the scratch
    none = torch.full_like(hit_p, EMPTY)
    assert float(median_hit_adjoint(state, ones, none, _fill=nan).abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------- 6. autograd and plumbing
def test_autograd_hands_the_depth_gradient_to_means3D_alone():
    from das3r_amd import median_depth_of, median_hit_adjoint
    name = "basic_deg3"
    sc, _, G = _scene(name)
    dev = _dev()
    G = G.to(dev)
    _, kw, state, geo = _render(name, dev)
    D, hit_g = median_depth_of(state, geometry=geo, return_hit=True)
    assert D.shape == (1, sc.H, sc.W) and D.requires_grad and not hit_g.requires_grad
    plain = median_depth_of(state, return_hit=True, return_position=True)
    assert torch.equal(D.detach(), plain[0]) and torch.equal(hit_g, plain[1]), "the planes are median_depth_of's own"
    (D * G).sum().backward()
    dz = median_hit_adjoint(state, G[0].contiguous(), plain[2])
    row = geo.raster_settings.viewmatrix.to(dev).float().reshape(4, 4)[:3, 2]
    assert float(row.abs().max()) > 0 and float(dz.abs().max()) > 0
    assert torch.equal(kw["means3D"].grad, dz[:, None] * row[None])
    for k, v in kw.items():
        if k != "means3D":
            assert v.grad is None, f"{k}: no other leaf gets a gradient"


def test_a_colour_loss_and_a_median_depth_loss_through_one_forward_add_up(monkeypatch):
    """Every leaf's gradient is the sum of the two taken separately, within one fp32 addition: autograd adds the two backward calls' results."""
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    from das3r_amd import median_depth_of
    name = "basic_deg3"
    sc, _, G = _scene(name)
    dev = _dev()
    dL, G = sc.dL_dpix.to(dev), G.to(dev)
    grads = []
    for terms in ((True, False), (False, True), (True, True)):
        out, kw, state, geo = _render(name, dev)
        D = median_depth_of(state, geometry=geo)
        loss = ((out[0] * dL).sum() if terms[0] else 0.0) + ((D * G).sum() if terms[1] else 0.0)
        loss.backward()
        grads.append({k: v.grad for k, v in kw.items()})
    colour, med, both = grads
    assert float(colour["means3D"].abs().max()) > 0 and float(med["means3D"].abs().max()) > 0
    a, b = colour["means3D"].double(), med["means3D"].double()
    assert bool(((both["means3D"].double() - (a + b)).abs() <= 2.0 ** -23 * (a.abs() + b.abs())).all())
    for k in ("opacities", "scales", "rotations", "means2D", "shs"):
        assert med[k] is None and torch.equal(both[k], colour[k]), k


def _small_model(seed=4):
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    seq = synthetic_sequence(frames=3, W=48, H=32, focal=44.0, n_splats=800, seed=seed)
    return build_from_sequence(copy.deepcopy(seq))


MODEL_PARAMS = ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation", "Q", "T")


def test_render_carries_both_keys_and_is_untouched_without_the_flag(monkeypatch):
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")   # (the pixel-per-lane backward meets its waves with LDS atomics: bit-equality needs the fixed order)
    from das3r_amd import _lib
    from das3r_amd.render import das3r_render
    model, cams = _small_model()
    bg = torch.zeros(3, device="cuda")
    dL = torch.randn(3, 32, 48, generator=torch.Generator().manual_seed(5)).cuda()
    runs = {}
    for on in (False, True):
        for p in MODEL_PARAMS:
            getattr(model, p).grad = None
        _lib.profile_report()
        _lib.profile_enable(True)
        pkg = das3r_render(cams[1], model, PIPE, bg, camera_pose=model.get_RT(1), **({"return_median_depth": True} if on else {}))
        (pkg["render"] * dL).sum().backward()
        torch.cuda.synchronize()
        _lib.profile_enable(False)
        ran = _lib.profile_report()
        launched = sorted(k for k in ran if k.startswith("render_median"))
        assert launched == (["render_median_forward_kernel"] if on else []), ran
        runs[on] = (pkg, {p: getattr(model, p).grad.clone() for p in MODEL_PARAMS if getattr(model, p).grad is not None},
                    pkg["viewspace_points"].grad.clone())
    (p0, g0, m0), (p1, g1, m1) = runs[False], runs[True]
    assert "median_depth" not in p0 and "median_hit" not in p0
    assert p1["median_depth"].shape == (1, 32, 48) and p1["median_depth"].requires_grad
    assert p1["median_hit"].shape == (32, 48) and p1["median_hit"].dtype == torch.int32 and int(p1["median_hit"].max()) >= 0
    assert torch.equal(p0["render"], p1["render"]) and torch.equal(p0["radii"], p1["radii"]) and torch.equal(m0, m1)
    assert set(g0) == set(g1) and "_xyz" in g0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    # and a loss on the median depth reaches the means and the pose
    for p in MODEL_PARAMS:
        getattr(model, p).grad = None
    pkg = das3r_render(cams[1], model, PIPE, bg, camera_pose=model.get_RT(1), return_median_depth=True)
    pkg["median_depth"].sum().backward()
    assert float(model._xyz.grad.abs().max()) > 0


def test_surface_scores_over_two_views_count_their_covered_pixels():
    from das3r_amd import alpha_of
    from das3r_amd.prune import surface_scores
    from das3r_amd.render import das3r_render
    model, cams = _small_model()
    bg = torch.zeros(3, device="cuda")
    views = cams[:2]
    variant = "render" if hasattr(model, "aggregated_mask") else "test"   # (surface_scores' own choice)
    scores = surface_scores(model, views, PIPE, bg)
    assert scores.shape == (model._xyz.shape[0],) and scores.dtype == torch.float32
    assert torch.equal(scores, scores.round()) and float(scores.min()) >= 0.0, "pixel counts"
    covered = 0
    with torch.no_grad():
        for v in views:
            state = das3r_render(v, model, PIPE, bg, camera_pose=model.get_RT(v.uid), variant=variant, return_state=True)["raster_state"]
            covered += int((alpha_of(state) > 0).sum())
    assert covered > 0 and float(scores.double().sum()) == float(covered)
    assert torch.equal(scores, surface_scores(model, views, PIPE, bg)), "bit-identical from run to run"
    assert bool((scores == 0).any()) and bool((scores > 0).any())


def test_render_set_writes_the_median_depth_maps(tmp_path):
    """What offline --median-depth does per view, in both render forms: the map is returned, written as median_depth/%05d.npy, positive exactly
    where something was blended, and its diagnostic against a depth map is the one --depth prints on the blended depth."""
    import numpy as np
    from das3r_amd import offline
    from tests.test_gpu_aux import _loaded_model
    model, cams = _loaded_model(W=48, H=32)
    for fused in (True, False):
        med, amaps, inv = [], [], []
        offline.render_set(str(tmp_path / str(fused)), "interp", 7, cams[:2], model, write=True, fused=fused, invdepth=inv, alpha=amaps, median_depth=med)
        assert len(med) == 2
        for idx, (z, a, i) in enumerate(zip(med, amaps, inv)):
            assert z.shape == (1, 32, 48) and z.dtype == torch.float32
            assert torch.equal(z > 0, a > 0), "a depth exactly where something was blended"
            arr = np.load(tmp_path / str(fused) / "interp" / "ours_7" / "median_depth" / f"{idx:05d}.npy")
            assert arr.shape == (32, 48) and arr.dtype == np.float32 and np.array_equal(arr, z[0].cpu().numpy())
            # both depth images against one map (here: the median depth itself) through the two diagnostics
            assert offline.median_depth_median_rel_error(z, z[0]) == 0.0
            assert 0.0 <= offline.invdepth_median_rel_error(i, z[0]) < 1.0
