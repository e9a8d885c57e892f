"""The launches of one forward, flow by flow: das3r_raster_forward (das3r_amd/csrc/forward.hip: ForwardCall) takes one of three flows — exact,
speculative, speculative with the emission fused into the preprocess kernel — over one of three binning paths, redoes its binning after an
overflow, may split its preprocess kernel, and may render an inverse-depth image.  Which kernels a forward launches, and how often, depends
on the call's shape and on the switches only, never on a timing: the per-kernel launch table (the library's own profiler, names with their
template arguments as the launch sites spell them) of exactly one forward + its backward must EQUAL the table written down here.

The tables below are literals.  They were recorded on an MI355X from the commit BEFORE the forward moved out of api.hip (docs/ledger.md
entry (cj)), not from the code under test: a step that went missing, ran twice or changed places with a differently named one shows here.
One host thread; every case starts with das3r_raster_forget_shapes, so the learnt state is that of a thread's first forward every time."""
import ctypes as C

import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

# case -> (scene, environment, forwards of the shape that run BEFORE the profiled one (scale modifiers), keyword switches)
CASES = {
    "first_forward_exact":          ("basic_deg3", {}, [], {}),
    "second_forward_fused_emit":    ("basic_deg3", {}, [1.0], {}),
    "first_forward_long_lists":     ("long_lists", {}, [], {}),
    "second_forward_long_lists":    ("long_lists", {}, [1.0], {}),
    "speculative_without_fused_emit": ("basic_deg3", {"DAS3R_FUSED_EMIT": "0"}, [1.0], {}),
    "global_sort_first":            ("basic_deg3", {"DAS3R_BINNING": "radix"}, [], {}),
    "global_sort_second":           ("basic_deg3", {"DAS3R_BINNING": "radix"}, [1.0], {}),
    "segmented_first":              ("basic_deg3", {"DAS3R_BINNING": "seg"}, [], {}),
    "segmented_second":             ("basic_deg3", {"DAS3R_BINNING": "seg"}, [1.0], {}),
    "overflow_redo":                ("long_lists", {"DAS3R_BINNING": "local"}, [0.15], {}),
    "split_preprocess_first":       ("basic_deg3", {"DAS3R_SPLIT_COLOUR": "1", "DAS3R_FUSED_EMIT": "0"}, [], {}),
    "split_preprocess_second":      ("basic_deg3", {"DAS3R_SPLIT_COLOUR": "1", "DAS3R_FUSED_EMIT": "0"}, [1.0], {}),
    "invdepth_first":               ("basic_deg3", {}, [], {"invdepth": True}),
    "invdepth_second":              ("basic_deg3", {}, [1.0], {"invdepth": True}),
    "debug_first":                  ("basic_deg3", {}, [], {"debug": True}),
    "debug_second":                 ("basic_deg3", {}, [1.0], {"debug": True}),
}

EXPECTED = {
    "first_forward_exact": {   # num_rendered 3642, capacity 3642
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "tile_ranges_kernel": 1,
    },
    "second_forward_fused_emit": {   # num_rendered 3642, capacity 8648
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_rows_kernel<false>": 1,
        "tile_ranges_kernel": 1,
    },
    "first_forward_long_lists": {   # num_rendered 17387, capacity 17387
        "depth_hist_kernel": 1,
        "list_skew_kernel": 1,
        "onesweep_pass_kernel<4, false>": 4,
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, false, false>": 1,
        "preprocess_kernel<true, false, false>": 1,
        "render_backward_regions_kernel<128, 5>": 1,
        "render_forward_regions_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "tile_lpt_kernel": 1,
        "tile_ranges_kernel": 1,
    },
    "second_forward_long_lists": {   # num_rendered 17387, capacity 25829
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, false, false>": 1,
        "preprocess_kernel<true, false, false>": 1,
        "render_backward_regions_kernel<128, 5>": 1,
        "render_forward_regions_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "segment_sort_kernel": 1,
        "tile_lpt_kernel": 1,
    },
    "speculative_without_fused_emit": {   # num_rendered 3642, capacity 8648
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_rows_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "tile_ranges_kernel": 1,
    },
    "global_sort_first": {   # num_rendered 3642, capacity 3642
        "depth_hist_kernel": 1,
        "onesweep_pass_kernel<4, false>": 4,
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "tile_ranges_kernel": 1,
    },
    "global_sort_second": {   # num_rendered 3642, capacity 3642
        "depth_hist_kernel": 1,
        "onesweep_pass_kernel<4, false>": 4,
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "tile_ranges_kernel": 1,
    },
    "segmented_first": {   # num_rendered 3642, capacity 3642
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "segment_sort_kernel": 1,
    },
    "segmented_second": {   # num_rendered 3642, capacity 8648
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_rows_kernel<true>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "segment_sort_kernel": 1,
    },
    "overflow_redo": {   # num_rendered 17387, capacity 17387
        "onesweep_pass_kernel<4, true>": 2,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, false, false>": 1,
        "preprocess_kernel<true, false, false>": 1,
        "render_backward_blk_kernel<192, 0, 0, 4, false>": 1,
        "render_forward_rows_kernel<false>": 2,
        "scan_emit_kernel<true, 1>": 1,
        "tile_ranges_kernel": 2,
    },
    "split_preprocess_first": {   # num_rendered 3642, capacity 3642
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_geometry_kernel<false, false>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "sh_colour_kernel<true>": 1,
        "tile_ranges_kernel": 1,
    },
    "split_preprocess_second": {   # num_rendered 3642, capacity 8648
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_geometry_kernel<false, false>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_rows_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "sh_colour_kernel<true>": 1,
        "tile_ranges_kernel": 1,
    },
    "invdepth_first": {   # num_rendered 3642, capacity 3642
        "depth_fold_kernel": 1,
        "depth_pass_inputs_kernel": 1,
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, true, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 2,
        "render_forward_kernel<true>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "tile_ranges_kernel": 1,
    },
    "invdepth_second": {   # num_rendered 3642, capacity 8648
        "depth_fold_kernel": 1,
        "depth_pass_inputs_kernel": 1,
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, true, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 2,
        "render_forward_rows_kernel<false, true>": 1,
        "tile_ranges_kernel": 1,
    },
    "debug_first": {   # num_rendered 3642, capacity 3642
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_kernel<false>": 1,
        "scan_emit_kernel<true, 1>": 1,
        "tile_ranges_kernel": 1,
    },
    "debug_second": {   # num_rendered 3642, capacity 8648
        "onesweep_pass_kernel<4, true>": 1,
        "preprocess_backward_kernel<true, false, false, true, false, false, false, true, false>": 1,
        "preprocess_kernel<true, false, true>": 1,
        "render_backward_kernel<true>": 1,
        "render_forward_rows_kernel<false>": 1,
        "tile_ranges_kernel": 1,
    },
}


def run_case(name, setenv):
    """-> ({kernel name: launches} of the case's one profiled forward + backward, (num_rendered, capacity) of that forward)."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    scene, env, before, kw = CASES[name]
    dev = torch.device("cuda:0")
    sc, _mode = util.scene_variant(scene)
    scd = sc.to(dev)
    skw = {**scd.settings_kwargs(), "debug": bool(kw.get("debug", False))}
    invdepth = bool(kw.get("invdepth", False))
    e = torch.empty(0, device=dev)
    for k, v in env.items():
        setenv(k, v)

    def forward(mod):
        rs = GaussianRasterizationSettings(**{**skw, "scale_modifier": mod})
        return rs, rasterizer._forward_full(rs, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e, invdepth=invdepth)

    _lib.forget_shapes()
    for mod in before:
        forward(mod)
    torch.cuda.synchronize()
    _lib.profile_report()   # drain
    _lib.profile_enable(True)
    try:
        rs, out = forward(1.0)
        I, _c, _r, g, b, i, cap = out[:7]
        grad_inv = torch.ones(1, sc.H, sc.W, device=dev) if invdepth else None
        rasterizer._backward_impl(rs, I, scd.dL_dpix, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e, g, b, i, cap,
                                  grad_invdepth=grad_inv)
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    return {k: n for k, (n, _ms) in _lib.profile_report(raw=True).items()}, (int(I), int(cap))


@pytest.mark.parametrize("name", list(CASES))
def test_one_forward_launches_what_it_always_did(name, monkeypatch):
    ran, (I, cap) = run_case(name, monkeypatch.setenv)
    print(f"{name}: num_rendered {I}, capacity {cap}\n  {ran}")
    if name == "overflow_redo":
        assert cap == I, "the redone forward is laid out exactly"
    elif name.endswith("first") or name.startswith("first"):
        assert cap == I, "a shape's first forward is laid out exactly"
    assert ran == EXPECTED[name]


def run_empty_scene():
    """P = 0 through the C entry itself (rasterizer._forward_full answers an empty scene without calling the library)."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    dev = torch.device("cuda:0")
    sc, _mode = util.scene_variant("basic_deg3")
    rs = GaussianRasterizationSettings(**sc.to(dev).settings_kwargs())
    keep = []
    a = rasterizer._fill_args(rs, 0, 0, dev, keep)
    color = torch.full((3, sc.H, sc.W), 7.0, device=dev)
    o = _lib.RasterOut()
    o.out_color = color.data_ptr()
    alloc = rasterizer._Alloc.get(dev)
    saved = _lib.RasterSaved()
    _lib.forget_shapes()
    _lib.profile_report()
    _lib.profile_enable(True)
    try:
        rc = _lib.load().das3r_raster_forward(C.byref(a), C.byref(_lib.RasterIn()), C.byref(o), alloc.fns["geom"], alloc.fns["binning"],
                                               alloc.fns["img"], None, C.byref(saved), rasterizer._stream(dev))
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    bufs = alloc.take()
    return rc, _lib.profile_report(raw=True), color, saved, bufs


def test_an_empty_scene_launches_nothing():
    rc, ran, color, saved, bufs = run_empty_scene()
    assert rc == 0 and ran == {}, (rc, ran)
    assert not color.any(), "upstream's empty scene: a zero image, the background not applied"
    assert saved.num_rendered == 0 and saved.capacity == 0 and saved.check_tag == 0
    assert set(bufs) == {"geom", "binning", "img"} and bufs["binning"].numel() == 256
