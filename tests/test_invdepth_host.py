"""CPU tests of the inverse-depth output's host side (ABI 16): the C struct, the argument checks that run before the device is touched,
the drop-in surface and the offline tool's --depth flag."""
import ctypes
import inspect

import torch


def test_abi_16_and_raster_out_layout(hip_lib):
    from das3r_amd import _lib
    assert _lib.ABI_VERSION == 16 and hip_lib.das3r_abi_version() == 16
    assert ctypes.sizeof(_lib.RasterOut) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.RasterOut.out_invdepth.offset == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert _lib.RasterOut().out_invdepth is None   # (a zero-filled struct: colour only, as before)


def test_slices_with_invdepth_is_refused_before_the_device(hip_lib, monkeypatch):
    """DAS3R_RENDER=slices has no inverse-depth form: a negative status and a message, before any allocation or launch."""
    from das3r_amd import _lib
    monkeypatch.setenv("DAS3R_RENDER", "slices")
    _lib.reload_switches()
    a, i, o, s = _lib.RasterArgs(), _lib.RasterIn(), _lib.RasterOut(), _lib.RasterSaved()
    a.P, a.image_width, a.image_height, a.M, a.sh_degree = 4, 32, 16, 0, 0
    a.tanfovx = a.tanfovy = 1.0
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: the call must stop at the argument checks
    a.bg = a.viewmatrix = a.projmatrix = a.campos = fake
    i.means3D = i.opacities = i.colors_precomp = i.scales = i.rotations = fake
    o.out_color = o.radii = o.out_invdepth = fake
    calls = []
    cb = _lib.ALLOC_FN(lambda u, n: calls.append(n) or 0)
    rc = hip_lib.das3r_raster_forward(ctypes.byref(a), ctypes.byref(i), ctypes.byref(o), cb, cb, cb, None, ctypes.byref(s), None)
    assert rc == -1 and b"slices has no inverse-depth form" in hip_lib.das3r_last_error()
    assert calls == [], "nothing may be allocated before the combination is refused"


def test_drop_in_surface_has_return_invdepth():
    from diff_gaussian_rasterization import GaussianRasterizer
    from das3r_amd.render import das3r_render
    p = inspect.signature(GaussianRasterizer.forward).parameters
    assert "return_invdepth" in p and p["return_invdepth"].default is False
    assert inspect.signature(das3r_render).parameters["return_invdepth"].default is False


def test_offline_depth_flag(monkeypatch):
    from das3r_amd import io_formats, offline
    seen = {}
    monkeypatch.setattr(io_formats, "load_sequence", lambda *a, **k: {"depths": None})
    monkeypatch.setattr(offline, "render_sets", lambda *a, **k: (seen.update(k), (7, []))[1])
    offline.main(["-m", "/nonexistent/model", "-s", "/nonexistent/seq", "--depth"])
    assert seen["depth"] is True
    offline.main(["-m", "/nonexistent/model", "-s", "/nonexistent/seq"])
    assert seen["depth"] is False
    sig = inspect.signature(offline.render_view_fused).parameters
    assert sig["invdepth"].default is False and inspect.signature(offline.render_set).parameters["invdepth"].default is None


def test_invdepth_median_rel_error():
    from das3r_amd.offline import invdepth_median_rel_error
    depth = torch.full((4, 5), 2.0)
    inv = torch.full((1, 4, 5), 0.5)
    inv[0, 0, :] = 0.0          # uncovered pixels do not count
    inv[0, 1, :] = 0.25         # 1 / 0.25 = 4: relative error 1
    assert abs(invdepth_median_rel_error(inv, depth) - 0.0) < 1e-7
    assert invdepth_median_rel_error(torch.zeros(1, 4, 5), depth) != invdepth_median_rel_error(torch.zeros(1, 4, 5), depth)   # NaN


def test_backward_depth_arguments_are_checked_before_the_device(hip_lib):
    """das3r_raster_backward_depth: a saved state without flags bit 1 (a colour-only forward, or flags = 0 handed back) is refused before
    anything is launched; so are missing upstream gradients.  Its scratch is the colour backward's rows twice."""
    from das3r_amd import _lib
    a, i, s, g = _lib.RasterArgs(), _lib.RasterIn(), _lib.RasterSaved(), _lib.RasterGrads()
    a.P, a.image_width, a.image_height, a.M, a.sh_degree = 4, 32, 16, 0, 0
    a.tanfovx = a.tanfovy = 1.0
    fake = ctypes.c_void_p(0x1000)   # never dereferenced
    a.bg = a.viewmatrix = a.projmatrix = a.campos = fake
    i.means3D = i.opacities = i.colors_precomp = i.scales = i.rotations = fake
    s.geom = s.binning = s.img = fake
    s.num_rendered = s.capacity = 10
    s.flags = 0
    g.dL_dmeans2D = g.dL_dopacities = g.dL_dmeans3D = g.dL_dcolors_precomp = g.dL_dscales = g.dL_drotations = g.scratch = fake
    rc = hip_lib.das3r_raster_backward_depth(ctypes.byref(a), ctypes.byref(i), ctypes.byref(s), fake, fake, ctypes.byref(g), None)
    assert rc == -1 and b"flags bit 1" in hip_lib.das3r_last_error()
    s.flags = 2
    rc = hip_lib.das3r_raster_backward_depth(ctypes.byref(a), ctypes.byref(i), ctypes.byref(s), fake, None, ctypes.byref(g), None)
    assert rc == -1 and b"das3r_raster_backward_depth" in hip_lib.das3r_last_error()
    for cap in (1, 1000, 123457):
        assert hip_lib.das3r_raster_backward_depth_scratch_bytes(cap) >= 2 * hip_lib.das3r_raster_backward_scratch_bytes(cap)
    assert hip_lib.das3r_raster_backward_scratch_bytes(1000) == 1000 * 36 + 16   # (unchanged)
