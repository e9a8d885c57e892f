"""The launch follows the choice: the compositing kernels a forward and a backward launch, unforced, are the ones
das3r_amd/csrc/kernel_choice.h chooses for the scene (das3r_debug_choose_forward / _backward on the scene's own numbers) and the ones written
down here — at a mean tile list below 96, in the hundreds, and from 1024 on.  Kernel names only (the library's own profiler); the parity
tests compare the numbers."""
import ctypes as C

import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

W = H = 32   # 2 x 2 tiles
NTILES = 4
FWD_PREFIX = {1: "render_forward_kernel", 2: "render_forward_rows", 3: "render_forward_lanes", 4: "render_forward_slices", 5: "render_forward_regions"}
BWD_PREFIX = {1: "render_backward_kernel", 3: "render_backward_scan", 6: "render_backward_blk", 7: "render_backward_regions"}


def _scene(name):
    """(a) `short`: 64 small splats, a mean list below 96; (b) `long` / (c) `longer`: 600 / 1100 splats that each cover the whole image, a mean
    list of exactly 600 / 1100 (>= 1024)."""
    if name == "short":
        return util.make_scene(P=64, W=W, H=H, focal=30.0, sh_degree=0, seed=71, s_px=(0.5, 2.0))
    P = {"long": 600, "longer": 1100}[name]
    focal = 30.0
    sc = util.make_scene(P=P, W=W, H=H, focal=focal, sh_degree=0, seed=72 + P, opacity=0.3)
    z = sc.means3D[:, 2:3]
    means3D = torch.cat([sc.means3D[:, :2] * 0.05, z], 1).contiguous()   # centres within a pixel or two of the image centre
    scales = (60.0 * z / focal).expand(-1, 3).contiguous()                # isotropic, sigma = 60 px: alpha >= 1/255 out to 2.9 sigma at opacity 0.3
    return util.Scene(**{**sc.__dict__, "means3D": means3D, "scales": scales})


def _forward_backward(sc):
    """One forward and one backward of a shape the library has not met (its binning buffer is then laid out for exactly num_rendered), under the
    profiler -> (kernels that ran, num_rendered, das3r_raster_saved.flags)."""
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib
    dev = torch.device("cuda:0")
    mode = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
    kw = {k: v.to(dev).clone().requires_grad_(True) for k, v in util.raster_inputs(sc, mode).items()}
    skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()}
    means2D = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    _lib.forget_shapes()
    _lib.profile_report()   # drain
    _lib.profile_enable(True)
    try:
        color, _ = GaussianRasterizer(GaussianRasterizationSettings(**skw))(means2D=means2D, **kw)
        fn = color.grad_fn
        color.backward(sc.dL_dpix.to(dev))
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    ran = _lib.profile_report()
    assert int(fn.capacity) == fn.num_rendered, "a shape's first forward lays its buffer out exactly"
    return ran, int(fn.num_rendered), int(fn.capacity.flags)


def _chosen(env, ran, num_rendered, flags):
    """-> (forward, backward) kernel-name prefixes kernel_choice.h chooses for these numbers under the switches `env` spells."""
    from das3r_amd import _lib
    lib = _lib.load()
    names = (C.c_char_p * max(len(env), 1))(*[k.encode() for k in env])
    values = (C.c_char_p * max(len(env), 1))(*[v.encode() for v in env.values()])
    sw, fwd, bwd = _lib.Switches(), _lib.FwdChoice(), _lib.BwdChoice()
    lib.das3r_debug_parse_switches(names, values, len(env), 0, C.byref(sw))
    local_lists = not any(k.startswith("depth_hist") for k in ran)   # no global depth sort ran: the lists reached the kernel in local order
    lib.das3r_debug_choose_forward(C.byref(sw), NTILES, num_rendered, int(local_lists), flags & 1, C.byref(fwd))
    lib.das3r_debug_choose_backward(C.byref(sw), num_rendered, NTILES, flags, C.byref(bwd))
    return FWD_PREFIX[fwd.kernel], BWD_PREFIX[bwd.kernel]


def _compositing(ran, direction):
    """The one compositing kernel of that direction that ran."""
    names = [k for k in ran if k.startswith("render_%s_" % direction)]
    assert len(names) == 1 and ran[names[0]][0] == 1, ran
    return names[0]


def _check(sc, env, want_fwd, want_bwd):
    ran, num_rendered, flags = _forward_backward(sc)
    fwd, bwd = _compositing(ran, "forward"), _compositing(ran, "backward")
    chosen_fwd, chosen_bwd = _chosen(env, ran, num_rendered, flags)
    print(f"num_rendered {num_rendered} flags {flags:#x}: ran {fwd} / {bwd}, chosen {chosen_fwd} / {chosen_bwd}")
    assert fwd.startswith(chosen_fwd) and bwd.startswith(chosen_bwd), (fwd, chosen_fwd, bwd, chosen_bwd)
    if callable(want_fwd):
        want_fwd, want_bwd = want_fwd(flags), want_bwd(flags)
    assert fwd.startswith(want_fwd) and bwd.startswith(want_bwd), (fwd, want_fwd, bwd, want_bwd)
    return num_rendered


def test_short_lists_take_the_pixel_per_lane_kernels():
    num_rendered = _check(_scene("short"), {}, "render_forward_kernel", "render_backward_kernel")
    assert 0 < num_rendered < 96 * NTILES


def test_lists_of_hundreds_take_the_row_forward_and_the_block_walk():
    sc = _scene("long")
    num_rendered = _check(sc, {}, "render_forward_rows", "render_backward_blk")
    assert num_rendered == sc.P * NTILES   # every splat in every tile: a mean list of 600


def test_lists_from_1024_on_take_a_workgroup_per_tile_or_four_as_the_forward_found_them():
    """Few tiles, long lists: the lanes forward and the block walk — or, where the forward's look at its lists found them skewed or crowded
    (flags bit 0), the 2x2-region kernels both ways."""
    sc = _scene("longer")
    num_rendered = _check(sc, {}, lambda flags: "render_forward_regions" if flags & 1 else "render_forward_lanes",
                          lambda flags: "render_backward_regions" if flags & 1 else "render_backward_blk")
    assert num_rendered == sc.P * NTILES   # a mean list of 1100


def test_deterministic_short_lists_take_the_block_walk(monkeypatch):
    from das3r_amd import _lib
    try:
        monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
        _lib.reload_switches()
        _check(_scene("short"), {"DAS3R_DETERMINISTIC": "1"}, "render_forward_kernel", "render_backward_blk")
    finally:
        monkeypatch.delenv("DAS3R_DETERMINISTIC", raising=False)
        _lib.reload_switches()
