"""Rasterizer parity on large tile grids (tests/tile_grid_scenes.py): strips of 255, 256 and 258 tiles on an axis (the packed rectangles'
last grid and the first two on the records path of the emission), 2^14 tiles, 3840 x 2160 (15 bits of tile id, one free key bit), a
16-bit grid (none) and a 17-bit grid (three partition passes) — each reached with a few thousand splats on a mostly empty image.

(a) every forced DAS3R_BINNING at every shape: per-Gaussian geometry, lists and ranges are the C oracle's bit for bit, and the plan that
    ran is the one tests/test_tile_grids_host.py derives from path_policy.h — never one read off a run;
(b) the unforced path: image and gradients against the oracle under the project's bars (tests/util.py, unchanged);
(c) every compositing kernel, forward and backward, sees the block -> tile map (render_common.h xcd_tile) of the records-path strip and of the 17-bit grid;
(d) a second, speculative forward of 3840 x 2160 and of the 17-bit grid leaves the same bits as the first;
(e) the saved-list kernels (feature composite, median depth) on the tall strip and the 17-bit grid;
(f) an image of 2^22 tiles is refused, by the library and by the Python layer, before anything is allocated or launched.
The largest accepted grid, 2^22 - 1 tiles, is over a billion pixels: out of scope here.

The oracle's forward + backward is computed once per shape and shared (tile_grid_scenes.oracle)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tile_grid_scenes as tg
from tests import util
from tests.test_gpu_bucket_local import GRADS, _dev, _view, assert_same_bits

pytestmark = pytest.mark.gpu

NAMES = list(tg.SHAPES)            # from the smallest grid to the largest
ORACLE_GRADS = ("means3D", "opacities", "shs", "scales", "rotations", "means2D")
FWD_KERNEL = {"quad": "render_forward_kernel", "rows": "render_forward_rows", "lanes": "render_forward_lanes", "fine": "render_forward_regions"}
BWD_KERNEL = {"dpp": "render_backward_kernel", "blk128": "render_backward_blk_kernel", "fine128": "render_backward_regions_kernel"}

_ON_DEVICE = {}


def _scene_on_device(name, long_list=True):
    key = (name, long_list)
    if key not in _ON_DEVICE:
        _ON_DEVICE[key] = tg.scene(name, long_list).to(_dev())
    return _ON_DEVICE[key]


def _align(n, a=256):
    return (n + a - 1) // a * a


def run(name, setenv, binning=None, rect_upstream=False, render=None, render_bwd=None, backward=True, before=0, exact=True, long_list=True, lists=True):
    """One forward (+ backward) of the shape's scene through the C entry under the given switches -> what it left behind, on the host, and the
    kernels it launched.  before: forwards of the same scene made first (the shape is forgotten before them)."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    dev = _dev()
    for var, value in (("DAS3R_BINNING", binning), ("DAS3R_RENDER", render), ("DAS3R_RENDER_BWD", render_bwd), ("DAS3R_RECT", "upstream" if rect_upstream else None)):
        if value is not None:
            setenv(var, value)
    scd = _scene_on_device(name, long_list)
    e = torch.empty(0, device=dev)
    rs = GaussianRasterizationSettings(**scd.settings_kwargs())
    forward = lambda ex: rasterizer._forward_full(rs, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e, exact=ex)
    _lib.forget_shapes()
    for _ in range(before):
        forward(True)
    torch.cuda.synchronize()
    _lib.profile_report()
    _lib.profile_enable(True)
    try:
        I, color, radii, geom, binning_buf, img, cap = forward(exact)[:7]
        grads = None
        if backward:
            grads = rasterizer._backward_impl(rs, I, scd.dL_dpix, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e, geom, binning_buf, img, cap)
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    ran = {k: n for k, (n, _ms) in _lib.profile_report().items()}
    W, H = tg.SHAPES[name]
    tx, ty = tg.grid(W, H)
    L = _lib.layout(scd.P, int(cap), W, H)
    res = dict(I=int(I), cap=int(cap), color=color.cpu(), radii=radii.cpu(), ran=ran, L=L,
               final_T=_view(img, L["final_T"], torch.int32, W * H).cpu(), n_contrib=_view(img, L["n_contrib"], torch.int32, W * H).cpu(),
               grads={k: t.cpu() for k, t in zip(GRADS, grads) if t is not None and t.numel()} if backward else {})
    if lists:
        res["point_list"] = _view(binning_buf, L["point_list"], torch.int32, int(I)).cpu().numpy().astype(np.uint32)
        res["ranges"] = _view(img, L["ranges"], torch.int32, 2 * tx * ty).cpu().numpy().reshape(tx * ty, 2).astype(np.uint32)
        res["geom"], res["binning"] = geom, binning_buf
    return res


def plan_that_ran(name, res):
    """(kind, onesweep_pass_kernel launches) of a forward, from its profile report.  The bucket plan and the local order launch the same
    kernels; what tells them apart is the partition key the last pass left behind (sort_onesweep.hip: keys ping-pong from the first of the
    binning buffer's arrays, one swap per pass): the last instance belongs to the last tile, and its key is the tile id under the local order,
    the tile id above the bucket and fraction bits — the key's top tbits — under the bucket plan."""
    ran = res["ran"]
    has = lambda prefix: any(k.startswith(prefix) for k in ran)
    sweeps = ran.get("onesweep_pass_kernel", 0)
    if has("cell_finish_kernel"):
        return "cells", sweeps
    if has("depth_hist"):
        return "radix", sweeps
    if has("segment_sort"):
        return "seg", sweeps
    tx, ty = tg.grid(*tg.SHAPES[name])
    tbits = tg.tile_bits(tx * ty)
    keys_at = 0 if sweeps % 2 == 0 else _align(4 * res["cap"])
    key = int(_view(res["binning"], keys_at, torch.int32, res["I"])[-1].item()) & 0xFFFFFFFF
    if key == tx * ty - 1:
        return "local", sweeps
    assert key >> (32 - tbits) == tx * ty - 1, f"{name}: the last partition key {key:#x} is neither the last tile's id nor that id above bucket bits"
    return "bucket", sweeps


# ----------------------------------------------------------------------------------------------------------------- (a) lists, bit for bit
def _assert_oracle_lists(name, res, what):
    """test_gpu_raster.py::test_binning_bit_exact's comparison: everything integer or exactly rounded equals the oracle's."""
    from das3r_amd import _lib
    sc = tg.scene(name)
    _, ref_radii, _, S = tg.oracle(name)
    P, L, geom = sc.P, res["L"], res["geom"]
    assert np.array_equal(res["radii"].numpy(), ref_radii), f"{what}: radii"
    vis = ref_radii > 0
    tt = _view(geom, L["tiles_touched"], torch.int32, P).cpu().numpy().astype(np.uint32)
    assert np.array_equal(tt, S["tiles_touched"]), f"{what}: tiles_touched"
    xy = _lib.splat_field(geom, L, "xy", P).cpu().numpy()[:, :2]
    co = _lib.splat_field(geom, L, "conic_opacity", P).cpu().numpy()
    rgbd = _lib.splat_field(geom, L, "rgbd", P).cpu().numpy()
    assert np.array_equal(xy[vis], S["xy"][vis]), f"{what}: pixel centres"
    assert np.array_equal(co[vis], S["conic_opacity"][vis]), f"{what}: conics and opacities"
    assert np.array_equal(rgbd[vis, 3], S["depths"][vis]) and np.array_equal(rgbd[vis, :3], S["rgb"][vis]), f"{what}: depths and SH colours"
    assert res["I"] == S["num_rendered"], f"{what}: num_rendered {res['I']} vs {S['num_rendered']}"
    bad = np.flatnonzero((res["ranges"] != S["ranges"]).any(1))
    assert bad.size == 0, f"{what}: ranges differ on {bad.size} tiles, the first {bad[:8]}"
    bad = np.flatnonzero(res["point_list"] != S["point_list"])
    assert bad.size == 0, f"{what}: point_list differs at {bad.size} positions, the first {bad[:8]}"
    W, H = tg.SHAPES[name]
    nc = res["n_contrib"].numpy().reshape(H, W).astype(np.uint32)
    assert (nc != S["n_contrib"]).mean() <= util.FLIP_FRACTION, f"{what}: n_contrib"


@pytest.mark.parametrize("switch", tg.SWITCHES)
@pytest.mark.parametrize("name", NAMES)
def test_forced_binning_is_bit_exact_and_takes_the_predicted_plan(name, switch, monkeypatch):
    res = run(name, monkeypatch.setenv, binning=switch, rect_upstream=True, backward=False)
    took, want = plan_that_ran(name, res), tg.REGIMES[name]["plans"][switch]
    print(f"{name} DAS3R_BINNING={switch}: num_rendered {res['I']}, took {took}, predicted {want}; {res['ran']}")
    assert took == want, f"{name} DAS3R_BINNING={switch}: took {took}, path_policy.h says {want}"
    _assert_oracle_lists(name, res, f"{name} {switch}")


def _subsequence_of(name, tight, upstream):
    """Every (tile, splat) instance of `tight` is one of `upstream`, in the same order inside its tile."""
    P = tg.scene(name).P

    def keys(r):
        tile = np.repeat(np.arange(r["ranges"].shape[0], dtype=np.int64), (r["ranges"][:, 1].astype(np.int64) - r["ranges"][:, 0].astype(np.int64)))
        return tile * P + r["point_list"].astype(np.int64)

    kt, ku = keys(tight), keys(upstream)
    order = np.argsort(ku, kind="stable")
    at = np.searchsorted(ku[order], kt)
    assert (at < ku.size).all() and np.array_equal(ku[order][np.minimum(at, ku.size - 1)], kt), "an instance upstream's square does not have"
    pos = order[at]
    assert (np.diff(pos) > 0).all(), "the order inside a tile changed"


@pytest.mark.parametrize("switch", tg.SWITCHES)
@pytest.mark.parametrize("name", ["wide256", "tall258", "three17"])
def test_default_rectangle_is_exact(name, switch, monkeypatch):
    """test_gpu_raster.py::test_tight_rect_is_exact on the records path: binning over the opacity-aware clipped rectangle only drops instances
    that contribute nowhere — the image is bit-identical to binning over upstream's square (under the rows kernel, which adds a pixel's terms
    one by one), the lists are upstream's with entries left out, the gradients equal up to the order of LDS adds — under the same plan."""
    up = run(name, monkeypatch.setenv, binning=switch, rect_upstream=True, render="rows")
    monkeypatch.delenv("DAS3R_RECT")
    tight = run(name, monkeypatch.setenv, binning=switch, render="rows")
    want = tg.REGIMES[name]["plans"][switch]
    assert plan_that_ran(name, up) == want and plan_that_ran(name, tight) == want
    print(f"{name} {switch}: num_rendered {tight['I']} of upstream's {up['I']}")
    assert tight["I"] <= up["I"] and tight["I"] == int(tight["ranges"][:, 1].astype(np.int64).max())
    assert torch.equal(tight["color"], up["color"]) and torch.equal(tight["radii"], up["radii"])
    _subsequence_of(name, tight, up)
    for k in up["grads"]:
        util.assert_grad_close(tight["grads"][k].numpy(), up["grads"][k].numpy(), f"{name} {switch}: tight vs upstream rect dL/d{k}", tol=1e-5)


# ---------------------------------------------------------------------------------------------------- (b) default path, image and gradients
def _assert_oracle_image_and_grads(name, res, what, kind=None):
    ref_color, ref_radii, ref_g, S = tg.oracle(name)
    assert np.array_equal(res["radii"].numpy(), ref_radii)
    assert 0 < res["I"] <= S["num_rendered"], "binned instances are a subset of upstream's"
    d = np.abs(res["color"].numpy().astype(np.float64) - ref_color)
    print(f"[{what}] colour: max |delta| {d.max():.3e}, {float((d > util.COLOR_TOL).mean()):.2e} of values beyond {util.COLOR_TOL} (bars {util.FLIP_MAX}, {util.FLIP_FRACTION})")
    util.assert_color_close(res["color"].numpy(), ref_color, f"{what} colour")
    bars = util.tolerances_for(kind)
    for k in ORACLE_GRADS:
        got, ref = res["grads"][k].numpy(), ref_g[k]
        rel = np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300)
        print(f"[{what}] dL/d{k}: max |delta| / max |ref| = {rel:.3e} (bar {bars['tol']})")
        util.assert_grad_close(got, ref, f"{what} dL/d{k}", tol=bars["tol"], flips=False)
        util.assert_grad_elementwise(got, ref, f"{what} dL/d{k}", rtol=bars["rtol"], floor=bars["floor"], outliers=bars["outliers"])
    assert float(res["grads"]["means2D"][:, 2].abs().max()) == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_default_path_image_and_gradients(name, monkeypatch):
    res = run(name, monkeypatch.setenv, lists=False)
    print(f"{name}: num_rendered {res['I']}; {res['ran']}")
    assert not any(k.startswith(("depth_hist", "segment_sort", "cell_finish")) for k in res["ran"]), "a shape's first forward takes the local order"
    assert res["ran"].get("onesweep_pass_kernel") == tg.REGIMES[name]["passes"]
    _assert_oracle_image_and_grads(name, res, name)


# -------------------------------------------------------------------------------------------------- (c) every kernel sees the tile map
@pytest.mark.parametrize("kind", list(FWD_KERNEL))
@pytest.mark.parametrize("name", ["wide256", "three17"])
def test_forward_kernels_on_the_tile_map(name, kind, monkeypatch):
    """(lists from the global sort: the local order's lists are composited by the kernels that can order them, whatever DAS3R_RENDER says)"""
    res = run(name, monkeypatch.setenv, binning="radix", render=kind, backward=False, lists=False)
    assert any(k.startswith(FWD_KERNEL[kind]) for k in res["ran"]), (kind, res["ran"])
    ref_color, ref_radii, _, _ = tg.oracle(name)
    assert np.array_equal(res["radii"].numpy(), ref_radii)
    util.assert_color_close(res["color"].numpy(), ref_color, f"{name} [{kind}] colour")


@pytest.mark.parametrize("kind", list(BWD_KERNEL))
@pytest.mark.parametrize("name", ["wide256", "three17"])
def test_backward_kernels_on_the_tile_map(name, kind, monkeypatch):
    res = run(name, monkeypatch.setenv, render_bwd=kind, lists=False)
    assert any(k.startswith(BWD_KERNEL[kind]) for k in res["ran"]), (kind, res["ran"])
    _assert_oracle_image_and_grads(name, res, f"{name} [{kind}]", kind)


# ------------------------------------------------------------------------------------------------------- (d) second forward of the shape
@pytest.mark.parametrize("switch", [None, "seg"])
@pytest.mark.parametrize("name", ["uhd", "three17"])
def test_second_forward_speculates_and_leaves_the_same_bits(name, switch, monkeypatch):
    """The scene without its list beyond LOCAL_MAX (such a list sends the shape's next forwards to the global sort, which does not speculate).
    No switch: the local order, its emission inside the preprocess kernel (preprocess.hip's digit loops); seg: the segmented path."""
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")   # (bit-identical gradients run to run: the block-walk backward, kernel_choice.h)
    first = run(name, monkeypatch.setenv, binning=switch, long_list=False)
    second = run(name, monkeypatch.setenv, binning=switch, long_list=False, before=1, exact=False)
    print(f"{name} {switch}: num_rendered {second['I']}, capacity {second['cap']}; {second['ran']}")
    assert second["cap"] > second["I"] == first["I"] == first["cap"], "the second forward speculates with headroom"
    if switch is None:
        assert not any(k.startswith("scan_emit_kernel") for k in second["ran"]), "the emission ran inside the preprocess kernel"
    else:
        assert any(k.startswith("segment_sort") for k in second["ran"])
    assert_same_bits(second, first, f"{name} {switch}: second forward vs first")


# ---------------------------------------------------------------------------------------------------------------- (e) saved-list kernels
@pytest.mark.parametrize("name", ["tall258", "three17"])
def test_feature_composite_against_the_colour_path(name):
    """Features = the colours: the composite is the colour image of the same forward (bg 0), and das3r_raster_aux_backward gives what
    das3r_raster_backward gives (tests/test_gpu_aux_geometry.py's check against the library's own colour path)."""
    from das3r_amd import GaussianRasterizationSettings, composite_features, feature_adjoint, rasterizer
    from tests.test_gpu_aux_geometry import _raw_aux_backward, _raw_forward
    dev = _dev()
    scd = _scene_on_device(name)
    kw = dict(means3D=scd.means3D, opacities=scd.opacities, scales=scd.scales, rotations=scd.rotations)
    rs = GaussianRasterizationSettings(**dict(scd.settings_kwargs(), bg=torch.zeros(3, device=dev)))
    cols = torch.rand(scd.P, 3, generator=torch.Generator().manual_seed(77)).to(dev)
    G3 = scd.dL_dpix
    res, state = _raw_forward(rs, kw, dev, cols)
    image = composite_features(state, cols)
    util.assert_color_close(image.cpu().numpy(), res[1].cpu().numpy(), f"{name}: composite of the colours vs the colour image")
    e = torch.empty(0, device=dev)
    ref = rasterizer._backward_impl(rs, res[0], G3, kw["means3D"], e, cols, kw["opacities"], kw["scales"], kw["rotations"], e, res[3], res[4], res[5], res[6])
    ref = dict(zip(("means2D", "features", "opacities", "means3D", "cov3D_precomp", "shs", "scales", "rotations"), ref))
    got = _raw_aux_backward(state, rs, kw, dev, cols, G3, None, colors=cols)
    for k in ("means3D", "opacities", "scales", "rotations", "means2D", "features"):
        util.assert_grad_close(got[k].cpu().numpy(), ref[k].cpu().numpy(), f"{name}: dL/d{k} vs the colour path")
    util.assert_grad_close(got["features"].cpu().numpy(), feature_adjoint(state, G3).cpu().numpy(), f"{name}: dL_dfeatures vs feature_adjoint")


MEDIAN_TILES = {   # stacks on both sides of row 255 | 256 and on the last tile / of column 255 | 256, of tile id 2^16 and on the last tile
    "tall258": [1, 254 * 3 + 1, 255 * 3 + 1, 256 * 3 + 1, 257 * 3 + 1, 3 * 258 - 1],
    "three17": [128 * 257 + 256, (1 << 16) - 1, 1 << 16, 257 * 256 - 1],
}


@pytest.mark.parametrize("name", ["tall258", "three17"])
def test_median_depth_against_the_reference(name):
    """tests/median_reference.py holds [pixels, splats] float64 matrices: stacks of four splats on a few tiles of the grid (tile_grid_scenes.stacked_scene)."""
    from das3r_amd import GaussianRasterizationSettings, rasterizer
    from tests import median_reference as mref
    from tests.test_gpu_median import _hold_to_reference
    dev = _dev()
    sc = tg.stacked_scene(name, MEDIAN_TILES[name])
    scd = sc.to(dev)
    e = torch.empty(0, device=dev)
    rs = GaussianRasterizationSettings(**scd.settings_kwargs())
    with torch.no_grad():
        res = rasterizer._forward_full(rs, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e)
        state = rasterizer.RasterState.of(res, rs)
        r = mref.reference_of_scene(sc, tg.MODE, 0.5, dev)
        depth, hit_g, _ = _hold_to_reference(state, r, 0.5, name)
    covered = hit_g >= 0
    W, H = tg.SHAPES[name]
    tx = tg.grid(W, H)[0]
    for t in MEDIAN_TILES[name]:
        y, x = min((t // tx) * 16 + 7, H - 1), min((t % tx) * 16 + 7, W - 1)   # (the last row of tiles of the strip is five pixels high)
        assert bool(covered[y, x]), f"{name}: the stack on tile {t} covers its centre"
    assert len(torch.unique(hit_g[covered])) > len(MEDIAN_TILES[name]), "the hit is not every stack's front splat"


# ------------------------------------------------------------------------------------------------------------------------- (f) refusal
def test_an_image_of_2_to_the_22_tiles_is_refused_before_anything_runs():
    """32768 x 32768 pixels are 2048 x 2048 = 2^22 tiles (render_common.h pack_tiles keeps 22 bits): DAS3R_ERR_INVALID_ARG with a message that
    names the limit, nothing allocated, nothing launched, the counters unchanged — from the library, and from the Python layer before it
    allocates the 12.9 GB image."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    from das3r_amd.synth import make_scene
    dev = _dev()
    lib = _lib.load()
    sc = make_scene(P=8, W=64, H=64, focal=50.0, sh_degree=1, seed=5).to(dev)
    rs = GaussianRasterizationSettings(**dict(sc.settings_kwargs(), image_width=32768, image_height=32768))
    keep = []
    a = rasterizer._fill_args(rs, sc.P, sc.shs.shape[1], dev, keep)
    a.capacity_hint = -1
    e = torch.empty(0, device=dev)
    i = rasterizer._fill_in(sc.means3D, sc.opacities, sc.shs, e, sc.scales, sc.rotations, e)
    color, radii = torch.zeros(3, 4, 4, device=dev), torch.zeros(sc.P, dtype=torch.int32, device=dev)   # (never written: the call is refused)
    o = _lib.RasterOut()
    o.out_color, o.radii = color.data_ptr(), radii.data_ptr()
    saved = _lib.RasterSaved()
    alloc = rasterizer._Alloc.get(dev)
    torch.cuda.synchronize()
    _lib.profile_report()
    _lib.profile_enable(True)
    before = _lib.stats()
    try:
        rc = lib.das3r_raster_forward(C.byref(a), C.byref(i), C.byref(o), alloc.fns["geom"], alloc.fns["binning"], alloc.fns["img"], None, C.byref(saved),
                                      rasterizer._stream(dev))
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    assert rc == _lib.ERR_INVALID_ARG
    assert "2^22" in _lib.last_error(), _lib.last_error()
    assert _lib.profile_report() == {} and _lib.stats() == before and alloc.take() == {}
    assert float(color.abs().max()) == 0.0
    # the Python layer
    allocated = torch.cuda.memory_allocated(dev)
    with pytest.raises(RuntimeError, match=r"status -1\).*2\^22 tiles"):
        rasterizer._forward_full(rs, sc.means3D, sc.shs, e, sc.opacities, sc.scales, sc.rotations, e)
    assert torch.cuda.memory_allocated(dev) == allocated and _lib.stats() == before
