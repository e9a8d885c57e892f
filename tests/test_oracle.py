"""CPU tests of the oracle itself (it is 'parity unpinned' by the reference — no reference test touches this path — so
it is pinned here three independent ways): C restatement vs the dense float64 autograd restatement, central finite
differences, and invariants of the algorithm."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle.dense_oracle import rasterize_dense
from tests import util

SMALL = ["basic_small", "deg0_small", "precomp_small", "cov_small", "world_small", "culled_small", "ties_small", "opaque_small",
         "edge_small", "portrait_small"]


def small_variant(name):
    from das3r_amd.synth import make_scene
    mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
    if name == "basic_small":
        sc = make_scene(P=220, W=52, H=37, focal=45.0, sh_degree=3, seed=41, bg=(0.2, 0.4, 0.1))
    elif name == "deg0_small":
        sc = make_scene(P=200, W=48, H=32, focal=40.0, sh_degree=0, seed=42)
    elif name == "precomp_small":
        sc = make_scene(P=200, W=48, H=32, focal=40.0, sh_degree=0, seed=43, bg=(1.0, 1.0, 1.0))
        mode["colors_precomp"] = True
    elif name == "cov_small":
        sc = make_scene(P=200, W=48, H=32, focal=40.0, sh_degree=1, seed=44)
        mode["cov3D_precomp"] = True
    elif name == "world_small":
        sc0, _ = util.scene_variant("world_camera")
        sc = make_scene(P=200, W=48, H=32, focal=40.0, sh_degree=2, seed=45)
        import math
        from das3r_amd.camera import projection_matrix
        view_col = util.look_at_view((0.3, -0.2, -0.8), (0.0, 0.1, 5.0))
        fovx, fovy = 2 * math.atan(sc.tanfovx), 2 * math.atan(sc.tanfovy)
        sc.viewmatrix = view_col.t().contiguous()
        sc.projmatrix = (view_col.t() @ projection_matrix(0.01, 100.0, fovx, fovy).t()).contiguous()
        sc.campos = torch.tensor([0.3, -0.2, -0.8])
        del sc0
    elif name == "culled_small":
        sc = make_scene(P=240, W=48, H=32, focal=40.0, sh_degree=1, seed=46)
        sc.means3D[:40, 2] = torch.linspace(-1.0, 0.002, 40)
        sc.means3D[40:80, 0] *= 4.0
    elif name == "ties_small":
        sc = make_scene(P=120, W=40, H=32, focal=36.0, sh_degree=0, seed=47, s_px=(1.0, 4.0))
        for fld in ("means3D", "scales", "rotations"):
            getattr(sc, fld)[60:] = getattr(sc, fld)[:60]
    elif name == "opaque_small":   # alpha clamp at 0.99 and the T < 1e-4 stop
        sc = make_scene(P=300, W=40, H=32, focal=36.0, sh_degree=1, seed=48, s_px=(3.0, 9.0))
        sc.opacities[:] = 0.999
        mode["scale_modifier"] = 1.0
    elif name == "edge_small":     # small util.scene_variant("frustum_edge"): unequal focals, 40 + 40 splats past the EWA clamp in x / in y
        sc = util.push_past_the_frustum_clamp(util.general_camera_scene(260, 56, 40, 50.0, 35.0, 2, 71), 40)
    elif name == "portrait_small":  # small util.scene_variant("portrait_world"): H > W, focal_x < focal_y, a view rotation with roll
        sc = util.general_camera_scene(220, 37, 60, 30.0, 48.0, 3, 72, view_col=util.rolled_view(), eye=util.ROLLED_EYE)
    else:
        raise KeyError(name)
    return sc, mode


def dense_run(sc, mode):
    inp = {k: v.double().clone().requires_grad_() for k, v in util.raster_inputs(sc, mode).items()}
    m2d = torch.zeros(sc.P, 3, dtype=torch.double, requires_grad=True)
    kw = {k: v for k, v in util.settings_kwargs(sc, mode).items() if k not in ("prefiltered", "debug")}
    out, radii, aux = rasterize_dense(means2D=m2d, **inp, **kw)
    (out * sc.dL_dpix.double()).sum().backward()
    g = {k: v.grad.numpy() for k, v in inp.items()}
    g["means2D"] = m2d.grad.numpy()
    return out.detach().numpy(), radii.numpy(), g, aux


@pytest.mark.parametrize("name", SMALL)
def test_c_oracle_matches_dense_autograd_oracle(name):
    sc, mode = small_variant(name)
    color, radii, g, S = util.run_oracle(sc, mode)
    d_color, d_radii, d_g, aux = dense_run(sc, mode)
    assert np.array_equal(radii, d_radii)
    util.assert_color_close(color, d_color, f"{name} colour (fp32 C vs fp64 dense)")
    gmap = {"means3D": "means3D", "opacities": "opacities", "shs": "shs", "scales": "scales", "rotations": "rotations",
            "means2D": "means2D", "colors_precomp": "colors", "cov3D_precomp": "cov3D"}
    for k, ref in d_g.items():
        util.assert_grad_close(g[gmap[k]], ref, f"{name} dL/d{k}", tol=1e-3)


def test_branches_of_appendix_a9_are_exercised():
    """The fixture set must actually hit the discrete branches it claims to."""
    sc, mode = small_variant("culled_small")
    _, radii, _, S = util.run_oracle(sc, mode, backward=False)
    assert (radii[:40] == 0).all() and (radii == 0).sum() > 40          # near cull + off-screen rects
    sc, mode = small_variant("opaque_small")
    _, _, _, S = util.run_oracle(sc, mode, backward=False)
    lens = (S["ranges"][:, 1] - S["ranges"][:, 0])
    assert (S["n_contrib"] < lens.max()).any() and S["final_T"].min() < 1e-3   # early stop reached
    sc, mode = util.scene_variant("long_lists")
    _, _, _, S = util.run_oracle(sc, mode, backward=False)
    assert (S["ranges"][:, 1] - S["ranges"][:, 0]).max() > 256               # multi-batch tile list
    sc, mode = util.scene_variant("basic_deg3")
    _, _, _, S = util.run_oracle(sc, mode, backward=False)
    assert S["clamped"].any()                                                # SH clamp (negative colour)
    # general cameras (util.CAMERA_VARIANTS): the two focal lengths apart, more tile rows than columns, the EWA frustum clamp on splats
    # that are rendered and carry a gradient that shows under the max-norm
    sc, mode = util.scene_variant("aniso_focal")
    fx, fy = sc.W / (2 * sc.tanfovx), sc.H / (2 * sc.tanfovy)
    assert abs(fx - fy) > 0.2 * min(fx, fy)
    sc, mode = util.scene_variant("portrait_world")
    assert (sc.H + 15) // 16 > (sc.W + 15) // 16
    sc, mode = util.scene_variant("frustum_edge")
    _, radii, g, S = util.run_oracle(sc, mode)
    flags = util.frustum_clamp_flags(sc)
    row = np.abs(g["means3D"]).max(1)
    for axis in range(2):
        hit = flags[:, axis] & (radii > 0)
        assert hit.sum() >= 50, (axis, int(hit.sum()))
        assert row[hit].max() >= 0.05 * row.max(), (axis, float(row[hit].max() / row.max()))
    assert (S["ranges"][:, 1] - S["ranges"][:, 0]).max() > 256               # and a tile list past one batch


def _with_focal_y_as_focal_x(sc):
    """The scene as a kernel would see it that took focal_x where focal_y belongs: tanfovy' = H tanfovx / W, written as make_scene writes
    a tangent — H / (2 focal) — so that a scene with equal focal lengths gets its own tanfovy back to the last bit."""
    from das3r_amd.synth import Scene
    focal_x = sc.W / (2.0 * sc.tanfovx)
    return Scene(**{**sc.__dict__, "tanfovy": sc.H / (2.0 * focal_x)})


def test_camera_variants_would_show_a_focal_swap():
    """Why util.CAMERA_VARIANTS exist: with focal_y := focal_x the oracle's image fails the colour bar and every geometry gradient moves by
    more than a hundred times the gradient bar on each of them — and on basic_deg3, as on every scene with equal focal lengths, by nothing."""
    geometry = ("means3D", "scales", "rotations", "means2D")
    for name in util.CAMERA_VARIANTS:
        sc, mode = util.scene_variant(name)
        color, _, g, _ = util.run_oracle(sc, mode)
        color_s, _, g_s, _ = util.run_oracle(_with_focal_y_as_focal_x(sc), mode)
        with pytest.raises(AssertionError):
            util.assert_color_close(color_s, color, f"{name} focal swap")
        for k in geometry:
            moved = np.abs(g_s[k] - g[k]).max() / np.abs(g[k]).max()
            assert moved > 100 * util.GRAD_REL_TOL, (name, k, float(moved))
    sc, mode = util.scene_variant("basic_deg3")
    swapped = _with_focal_y_as_focal_x(sc)
    assert swapped.tanfovy == sc.tanfovy, "equal focal lengths: the swap hands the oracle the very same number"
    color, radii, g, S = util.run_oracle(sc, mode)
    color_s, radii_s, g_s, S_s = util.run_oracle(swapped, mode)
    assert np.array_equal(color, color_s) and np.array_equal(radii, radii_s)
    for k in ("xy", "conic_opacity", "depths", "rgb", "point_list", "ranges", "n_contrib", "final_T"):
        assert np.array_equal(S[k], S_s[k]), k
    # (the two calls had the same inputs to the bit.  The C oracle's backward meets its tiles in float atomics, so two runs of ONE scene differ
    #  in the order of those additions: the gradients are held to the bar below which no parity test sees a change, not to equal bits)
    for k in g:
        util.assert_grad_close(g_s[k], g[k], f"basic_deg3 focal swap dL/d{k}")


def test_dense_oracle_finite_differences():
    """Central finite differences (float64, h = 1e-6) on the dense oracle: validates that what autograd differentiates is
    the function the forward computes (away from the non-differentiable thresholds)."""
    from das3r_amd.synth import make_scene
    sc = make_scene(P=60, W=32, H=24, focal=28.0, sh_degree=2, seed=51, s_px=(2.0, 5.0), opacity=0.35)
    mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
    kw = {k: v for k, v in util.settings_kwargs(sc, mode).items() if k not in ("prefiltered", "debug")}
    base = {k: v.double() for k, v in util.raster_inputs(sc, mode).items()}
    w = sc.dL_dpix.double() * (sc.W * sc.H)

    def f(vals):
        out, _, _ = rasterize_dense(means2D=torch.zeros(sc.P, 3, dtype=torch.double), **vals, **kw)
        return float((out * w).sum())

    leaves = {k: v.clone().requires_grad_() for k, v in base.items()}
    out, _, _ = rasterize_dense(means2D=torch.zeros(sc.P, 3, dtype=torch.double), **leaves, **kw)
    (out * w).sum().backward()
    g = torch.Generator().manual_seed(9)
    for k in base:
        d = torch.randn(base[k].shape, generator=g, dtype=torch.double)
        d = d / d.norm()
        h = 1e-6
        plus, minus = dict(base), dict(base)
        plus[k] = base[k] + h * d
        minus[k] = base[k] - h * d
        fd = (f(plus) - f(minus)) / (2 * h)
        an = float((leaves[k].grad * d).sum())
        assert abs(fd - an) <= 1e-4 * max(abs(fd), abs(an)) + 1e-7, f"{k}: fd {fd:.8e} vs autograd {an:.8e}"


def test_invariants_of_the_algorithm():
    sc, mode = util.scene_variant("basic_deg3")
    c0, r0, _, S0 = util.run_oracle(sc, mode, backward=False)
    # (1) background linearity: out = C + T_final * bg
    sc2, _ = util.scene_variant("basic_deg3")
    sc2.bg = torch.tensor([0.9, 0.0, 0.5])
    c1, _, _, S1 = util.run_oracle(sc2, mode, backward=False)
    dbg = (sc2.bg - sc.bg).numpy()
    np.testing.assert_allclose(c1 - c0, S0["final_T"][None] * dbg[:, None, None], atol=2e-7)
    # (2) permuting the input Gaussians leaves the image unchanged (no depth ties in this scene)
    perm = torch.randperm(sc.P, generator=torch.Generator().manual_seed(3))
    sc3, _ = util.scene_variant("basic_deg3")
    for fld in ("means3D", "scales", "rotations", "opacities", "shs"):
        setattr(sc3, fld, getattr(sc3, fld)[perm].contiguous())
    c3, r3, _, _ = util.run_oracle(sc3, mode, backward=False)
    assert np.array_equal(c3, c0) and np.array_equal(r3, r0[perm.numpy()])
    # (3) colours precomputed from the oracle's own SH stage reproduce the SH path exactly
    from oracle import c_oracle as co
    o = co.RasterOracle(**sc.settings_kwargs())
    c4, _ = o.forward(sc.means3D.numpy(), sc.opacities.numpy(), colors_precomp=S0["rgb"], scales=sc.scales.numpy(),
                      rotations=sc.rotations.numpy())
    assert np.array_equal(c4, c0)
    # (4) cov3D precomputed with the reference's Python-side formula reproduces the scale/rotation path
    c5, r5 = o.forward(sc.means3D.numpy(), sc.opacities.numpy(), shs=sc.shs.numpy(), cov3D_precomp=util.cov3d_of(sc).numpy())
    assert (r5 != r0).mean() < 0.01
    util.assert_color_close(c5, c0, "cov3D_precomp path")
    # (5) radii > 0  <=>  tiles_touched > 0
    assert np.array_equal(r0 > 0, S0["tiles_touched"] > 0)
    o.free()


def test_knn_oracle_matches_kdtree():
    from scipy.spatial import cKDTree
    g = np.random.default_rng(5)
    pts = g.random((3000, 3)).astype(np.float32)
    pts[100:110] = pts[0]                       # duplicates count with distance 0
    got = c_oracle.knn3_mean_dist2(pts)
    d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4)
    ref = (d[:, 1:] ** 2).mean(1)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-9)
    assert got[0] == 0.0


def test_mark_visible_oracle():
    sc, _ = small_variant("culled_small")
    vis = c_oracle.mark_visible(sc.means3D.numpy(), sc.viewmatrix.numpy(), sc.projmatrix.numpy())
    assert np.array_equal(vis, sc.means3D[:, 2].numpy() > 0.001)
