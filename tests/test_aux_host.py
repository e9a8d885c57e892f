"""Host-side tests of the aux-channel entry points (include/das3r_raster.h das3r_raster_aux_forward / _scratch_bytes / _adjoint) and of
their Python surface (das3r_amd.rasterizer RasterState / composite_features / feature_adjoint / alpha_of).  No device is needed: the
arguments are refused before anything is launched.  The kernels themselves: tests/test_gpu_aux.py."""
import ctypes as C
import inspect
import os

import pytest
import torch


def _args(P=10, W=32, H=16):
    from das3r_amd import _lib
    a = _lib.RasterArgs()
    a.P, a.image_width, a.image_height = P, W, H
    return a


def test_library_exports_the_aux_entry_points_under_abi_16(hip_lib):
    from das3r_amd import _lib
    for name in ("das3r_raster_aux_forward", "das3r_raster_aux_scratch_bytes", "das3r_raster_aux_adjoint"):
        assert hasattr(hip_lib, name) and name in _lib.EXPORTS
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    assert _lib.AUX_MAX_CHANNELS == 8
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "das3r_raster.h")) as f:
        header = f.read()
    assert "#define DAS3R_ABI_VERSION 16" in header and "#define DAS3R_AUX_MAX_CHANNELS 8" in header


def test_scratch_bytes_is_monotone_and_holds_a_row_per_instance(hip_lib):
    f = hip_lib.das3r_raster_aux_scratch_bytes
    caps = [0, 1, 2, 255, 256, 257, 100000, 1 << 24, 0x7FFFFF00]
    for c in range(1, 9):
        sizes = [f(cap, c) for cap in caps]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (c, sizes)
        assert all(s >= 4 * c * cap for s, cap in zip(sizes, caps)), (c, sizes)
    for cap in caps:
        sizes = [f(cap, c) for c in range(1, 9)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (cap, sizes)


@pytest.mark.parametrize("bad_c", [0, 9, -1])
def test_a_bad_channel_count_is_refused_with_a_message(hip_lib, bad_c):
    from das3r_amd import _lib
    a, saved = _args(), _lib.RasterSaved()
    p = C.c_void_p(64)   # (never dereferenced: the call fails first)
    assert hip_lib.das3r_raster_aux_forward(C.byref(a), C.byref(saved), bad_c, p, p, None) == -1
    assert b"das3r_raster_aux_forward" in hip_lib.das3r_last_error() and b"channels" in hip_lib.das3r_last_error()
    assert hip_lib.das3r_raster_aux_adjoint(C.byref(a), C.byref(saved), bad_c, p, p, 0, p, None) == -1
    assert b"das3r_raster_aux_adjoint" in hip_lib.das3r_last_error() and b"channels" in hip_lib.das3r_last_error()


def test_null_pointers_are_refused_with_a_message(hip_lib):
    from das3r_amd import _lib
    a, saved = _args(), _lib.RasterSaved()
    saved.num_rendered = saved.capacity = 100
    p = C.c_void_p(64)
    L = hip_lib
    assert L.das3r_raster_aux_forward(None, C.byref(saved), 1, p, p, None) == -1 and b"das3r_raster_aux_forward" in L.das3r_last_error()
    assert L.das3r_raster_aux_forward(C.byref(a), None, 1, p, p, None) == -1 and b"das3r_raster_aux_forward" in L.das3r_last_error()
    assert L.das3r_raster_aux_forward(C.byref(a), C.byref(saved), 1, None, p, None) == -1 and b"null" in L.das3r_last_error()
    assert L.das3r_raster_aux_forward(C.byref(a), C.byref(saved), 1, p, None, None) == -1 and b"null" in L.das3r_last_error()
    assert L.das3r_raster_aux_forward(C.byref(a), C.byref(saved), 1, p, p, None) == -1 and b"saved buffers" in L.das3r_last_error()
    assert L.das3r_raster_aux_adjoint(None, C.byref(saved), 1, p, p, 0, p, None) == -1 and b"das3r_raster_aux_adjoint" in L.das3r_last_error()
    assert L.das3r_raster_aux_adjoint(C.byref(a), C.byref(saved), 1, None, p, 0, p, None) == -1 and b"null" in L.das3r_last_error()
    assert L.das3r_raster_aux_adjoint(C.byref(a), C.byref(saved), 1, p, None, 0, p, None) == -1 and b"null" in L.das3r_last_error()
    assert L.das3r_raster_aux_adjoint(C.byref(a), C.byref(saved), 1, p, p, 0, p, None) == -1 and b"saved buffers" in L.das3r_last_error()
    saved.geom = saved.binning = saved.img = 64
    assert L.das3r_raster_aux_adjoint(C.byref(a), C.byref(saved), 1, p, p, 0, None, None) == -1 and b"scratch" in L.das3r_last_error()
    a.image_width = 0
    assert L.das3r_raster_aux_forward(C.byref(a), C.byref(saved), 1, p, p, None) == -1 and b"extents" in L.das3r_last_error()


def _state(P=10, W=32, H=16):
    """A state as a forward on a HIP device would leave it (the buffers are never touched: every call below fails first)."""
    from das3r_amd.rasterizer import RasterState
    e = torch.empty(0, dtype=torch.uint8)
    return RasterState(e, e, e, 0, 0, P, W, H, torch.device("cuda", 0))


def test_composite_features_refuses_what_it_cannot_take():
    from das3r_amd import composite_features
    st = _state()
    with pytest.raises(TypeError, match="float32"):
        composite_features(st, torch.zeros(10, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="11 rows.*10 Gaussians"):
        composite_features(st, torch.zeros(11, 3))
    with pytest.raises(ValueError, match="dimensions"):
        composite_features(st, torch.zeros(10))
    with pytest.raises(ValueError, match="contiguous"):
        composite_features(st, torch.zeros(3, 10).t())
    with pytest.raises(RuntimeError, match="is on cpu, the forward ran on cuda:0"):
        composite_features(st, torch.zeros(10, 3))
    with pytest.raises(TypeError, match="RasterState"):
        composite_features(object(), torch.zeros(10, 3))


def test_feature_adjoint_refuses_what_it_cannot_take():
    from das3r_amd import feature_adjoint
    st = _state()
    with pytest.raises(TypeError, match="float32"):
        feature_adjoint(st, torch.zeros(1, 16, 32, dtype=torch.float16))
    with pytest.raises(ValueError, match="dimensions"):
        feature_adjoint(st, torch.zeros(1, 32, 16))
    with pytest.raises(RuntimeError, match="is on cpu"):
        feature_adjoint(st, torch.zeros(1, 16, 32))
    with pytest.raises(ValueError, match="needs the tensor to add to"):
        feature_adjoint(_state_cpu(), torch.zeros(1, 16, 32), accumulate=True)
    with pytest.raises(ValueError, match="2 channels, grad_image 1"):
        feature_adjoint(_state_cpu(), torch.zeros(1, 16, 32), out=torch.zeros(10, 2))
    with pytest.raises(ValueError, match="contiguous"):
        feature_adjoint(_state_cpu(), torch.zeros(2, 16, 32), out=torch.zeros(2, 10).t())


def _state_cpu():
    """Device checks pass on it, so that the checks behind them can be reached without a device (nothing is ever launched on it)."""
    from das3r_amd.rasterizer import RasterState
    e = torch.empty(0, dtype=torch.uint8)
    return RasterState(e, e, e, 0, 0, 10, 32, 16, torch.device("cpu"))


def test_rasterizer_forward_keeps_its_signature_and_arity_by_default():
    from das3r_amd import GaussianRasterizer
    from das3r_amd.render import das3r_render
    from das3r_amd.offline import render_set, render_view_fused
    from das3r_amd.train import psnr_report
    sig = inspect.signature(GaussianRasterizer.forward)
    names = list(sig.parameters)
    # today's parameters, in today's order, then the two new keywords with defaults that change nothing
    assert names == ["self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "return_invdepth",
                     "antialiasing", "features", "return_alpha"]
    assert sig.parameters["features"].default is None and sig.parameters["return_alpha"].default is False
    assert sig.parameters["return_invdepth"].default is False and sig.parameters["antialiasing"].default is False
    for fn, kws in ((das3r_render, {"features": None, "return_alpha": False}), (render_view_fused, {"features": None, "alpha": False}),
                    (render_set, {"static_map": None, "alpha": None}), (psnr_report, {"static_mask": "gt", "static_threshold": 0.5})):
        p = inspect.signature(fn).parameters
        for k, v in kws.items():
            assert k in p and p[k].default == v, (fn.__name__, k)


def test_default_forward_returns_two_results_and_never_asks_for_the_state(monkeypatch):
    """With features / return_alpha at their defaults the call goes the way it went: the autograd function is applied once, is not asked to
    keep the state, and (color, radii) come back as they are."""
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer, rasterizer
    seen = {}

    def fake(*a, antialiasing=False, options=None):
        seen["want_state"] = options.want_state
        seen["calls"] = seen.get("calls", 0) + 1
        return torch.zeros(3, 4, 4), torch.zeros(5, dtype=torch.int32)

    monkeypatch.setattr(rasterizer, "rasterize_gaussians", fake)
    rs = GaussianRasterizationSettings(4, 4, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    z = torch.zeros(5, 3)
    r = GaussianRasterizer(rs)
    out = r(means3D=z, means2D=z, opacities=torch.zeros(5, 1), colors_precomp=z, scales=z, rotations=torch.zeros(5, 4))
    assert isinstance(out, tuple) and len(out) == 2 and seen == {"want_state": False, "calls": 1} and r.state is None


def test_parsers_take_the_flags():
    from das3r_amd import offline
    a = offline.parser().parse_args(["-m", "x", "-s", "y", "--static-map", "--alpha"])
    assert a.static_map and a.alpha
    a = offline.parser().parse_args(["-m", "x", "-s", "y"])
    assert not a.static_map and not a.alpha


def test_psnr_report_refuses_an_unknown_static_mask():
    from das3r_amd.train import psnr_report
    with pytest.raises(ValueError, match='"gt" or "rendered"'):
        psnr_report(None, [], static_mask="predicted")
