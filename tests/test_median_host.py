"""Host-side tests of the median-depth entry points (include/das3r_raster.h das3r_raster_median_forward / _median_scratch_bytes /
_median_adjoint) and of their Python surface (das3r_amd.median_depth_of, median_hit_adjoint, das3r_render(return_median_depth=),
prune.surface_scores, offline --median-depth).  No device is needed: the arguments are refused before anything is launched.  The kernels:
tests/test_gpu_median.py."""
import ctypes as C
import inspect
import os

import pytest
import torch

INVALID = -1   # DAS3R_ERR_INVALID_ARG
NAMES = ("das3r_raster_median_forward", "das3r_raster_median_scratch_bytes", "das3r_raster_median_adjoint")


def _structs(W=32):
    from das3r_amd import _lib
    args = _lib.RasterArgs()
    args.P, args.image_width, args.image_height = 10, W, 16
    sv = _lib.RasterSaved()
    sv.num_rendered = sv.capacity = 100
    return args, sv


def _forward(hip_lib, a="ok", saved="ok", depth="p", tau=0.5, W=32):
    """das3r_raster_median_forward on pointers that are never dereferenced: every call here fails first."""
    p = C.c_void_p(64)
    args, sv = _structs(W)
    return hip_lib.das3r_raster_median_forward(C.byref(args) if a == "ok" else None, C.byref(sv) if saved == "ok" else None, C.c_float(tau),
                                               p if depth == "p" else None, None, None, None)


def _adjoint(hip_lib, a="ok", saved="ok", dL="p", pos="p", dz="p", scratch="p", W=32):
    p = C.c_void_p(64)
    args, sv = _structs(W)
    pick = lambda v: p if v == "p" else None
    return hip_lib.das3r_raster_median_adjoint(C.byref(args) if a == "ok" else None, C.byref(sv) if saved == "ok" else None, pick(dL), pick(pos),
                                               pick(dz), 0, pick(scratch), None)


def test_library_exports_the_entry_points_under_abi_16(hip_lib):
    from das3r_amd import _lib
    for name in NAMES:
        assert hasattr(hip_lib, name) and name in _lib.EXPORTS
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "das3r_raster.h")) as f:
        header = f.read()
    assert "#define DAS3R_ABI_VERSION 16" in header
    assert "int das3r_raster_median_forward(" in header and "int das3r_raster_median_adjoint(" in header
    assert "size_t das3r_raster_median_scratch_bytes(" in header
    # the definition is fixed there
    for text in ("T_0 = 1, T_{k+1} = T_k (1 - alpha_k)", "hit = max { k < n : T_k > tau }", "An empty pixel is one with n_contrib == 0",
                 "0 < tau < 1", "held fixed", "No floating-point atomics, no unordered adds"):
        assert text in header, text


def test_scratch_bytes_is_monotone_and_holds_a_float_per_list_entry(hip_lib):
    f = hip_lib.das3r_raster_median_scratch_bytes
    caps = [0, 1, 2, 255, 256, 257, 100000, 1 << 24, 0x7FFFFF00]
    sizes = [f(cap) for cap in caps]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    assert all(s >= 4 * max(cap, 1) for s, cap in zip(sizes, caps)), sizes
    assert sizes == [hip_lib.das3r_raster_aux_scratch_bytes(cap, 1) for cap in caps], "the aux adjoint's rows at C = 1"


def test_every_listed_refusal_of_the_forward_comes_with_a_message(hip_lib):
    err = hip_lib.das3r_last_error
    who = b"das3r_raster_median_forward"
    for kw in ({"a": None}, {"saved": None}, {"depth": None}):
        assert _forward(hip_lib, **kw) == INVALID and who in err() and b"null" in err(), kw
    assert _forward(hip_lib, W=0) == INVALID and who in err() and b"extents" in err()
    for tau in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert _forward(hip_lib, tau=tau) == INVALID and who in err() and b"threshold" in err(), tau
    assert _forward(hip_lib) == INVALID and who in err() and b"saved buffers missing" in err()


def test_every_listed_refusal_of_the_adjoint_comes_with_a_message(hip_lib):
    err = hip_lib.das3r_last_error
    who = b"das3r_raster_median_adjoint"
    for kw in ({"a": None}, {"saved": None}):
        assert _adjoint(hip_lib, **kw) == INVALID and who in err() and b"null" in err(), kw
    assert _adjoint(hip_lib, dL=None) == INVALID and who in err() and b"dL_ddepth" in err()
    assert _adjoint(hip_lib, pos=None) == INVALID and who in err() and b"hit_position" in err()
    assert _adjoint(hip_lib, dz=None) == INVALID and who in err() and b"dL_dz" in err()
    assert _adjoint(hip_lib, scratch=None) == INVALID and who in err() and b"das3r_raster_median_scratch_bytes" in err()
    assert _adjoint(hip_lib, W=0) == INVALID and who in err() and b"extents" in err()
    assert _adjoint(hip_lib) == INVALID and who in err() and b"saved buffers missing" in err()


def _settings(W=32, H=16):
    from das3r_amd import GaussianRasterizationSettings
    return GaussianRasterizationSettings(H, W, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)


def _state(device, P=10, W=32, H=16):
    from das3r_amd.rasterizer import RasterState
    e = torch.empty(0, dtype=torch.uint8)
    return RasterState(e, e, e, 0, 0, P, W, H, torch.device(device))


def _geometry(P=10, W=32, H=16, **over):
    from das3r_amd import AuxGeometry
    kw = dict(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), colors_precomp=torch.zeros(P, 3),
              scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4))
    kw.update(over)
    return AuxGeometry(_settings(W, H), **kw)


def test_the_functions_are_exported_beside_distortion_of():
    import das3r_amd
    from das3r_amd import rasterizer
    assert das3r_amd.median_depth_of is rasterizer.median_depth_of and "median_depth_of" in das3r_amd.__all__
    assert das3r_amd.median_hit_adjoint is rasterizer.median_hit_adjoint and "median_hit_adjoint" in das3r_amd.__all__
    p = inspect.signature(das3r_amd.median_depth_of).parameters
    assert list(p)[:4] == ["state", "geometry", "threshold", "return_hit"]
    assert p["geometry"].default is None and p["threshold"].default == 0.5 and p["return_hit"].default is False
    p = inspect.signature(das3r_amd.median_hit_adjoint).parameters
    assert list(p)[:5] == ["state", "grad_image", "hit_position", "out", "accumulate"] and p["out"].default is None and p["accumulate"].default is False


def _no_library(monkeypatch):
    from das3r_amd import _lib

    def load():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", load)


def test_median_depth_of_refuses_what_it_cannot_take(monkeypatch):
    from das3r_amd import median_depth_of
    _no_library(monkeypatch)
    st = _state("cuda:0")   # (never touched: every call below fails first)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold must be inside \\(0, 1\\)"):
            median_depth_of(st, threshold=bad)
        with pytest.raises(ValueError, match="threshold must be inside \\(0, 1\\)"):
            median_depth_of(st, geometry=_geometry(), threshold=bad)
    with pytest.raises(TypeError, match="threshold must be a number"):
        median_depth_of(st, threshold="half")
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        median_depth_of(_state("cpu"))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        median_depth_of(_state("cpu"), geometry=_geometry())
    with pytest.raises(TypeError, match="AuxGeometry"):
        median_depth_of(_state("cpu"), geometry=object())
    with pytest.raises(TypeError, match="RasterState"):
        median_depth_of(object())
    with pytest.raises(TypeError, match="RasterState"):
        median_depth_of(object(), geometry=_geometry())
    with pytest.raises(ValueError, match="48 x 16, the forward rendered 32 x 16"):
        median_depth_of(st, geometry=_geometry(W=48))
    with pytest.raises(ValueError, match="geometry.means3D must be the forward's own tensor \\(10 rows\\)"):
        median_depth_of(st, geometry=_geometry(means3D=torch.zeros(11, 3)))
    with pytest.raises(RuntimeError, match="geometry.means3D is on cpu, the forward ran on cuda:0"):
        median_depth_of(st, geometry=_geometry())


def test_median_hit_adjoint_refuses_what_it_cannot_take(monkeypatch):
    from das3r_amd import median_hit_adjoint
    _no_library(monkeypatch)
    cpu = _state("cpu")
    g, pos = torch.zeros(16, 32), torch.zeros(16, 32, dtype=torch.int32)
    with pytest.raises(TypeError, match="RasterState"):
        median_hit_adjoint(object(), g, pos)
    with pytest.raises(TypeError, match="grad_image must be float32"):
        median_hit_adjoint(cpu, g.double(), pos)
    with pytest.raises(ValueError, match="grad_image must have dimensions \\(16, 32\\)"):
        median_hit_adjoint(cpu, torch.zeros(3, 16, 32), pos)
    with pytest.raises(TypeError, match="hit_position must be int32"):
        median_hit_adjoint(cpu, g, pos.long())
    with pytest.raises(TypeError, match="hit_position must be int32"):
        median_hit_adjoint(cpu, g, pos.float())
    with pytest.raises(TypeError, match="hit_position must be the int32"):
        median_hit_adjoint(cpu, g, None)
    for shape in ((32, 16), (1, 16, 32), (16, 31), (16 * 32,)):
        with pytest.raises(ValueError, match="hit_position must have dimensions \\(16, 32\\)"):
            median_hit_adjoint(cpu, g, torch.zeros(*shape, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs the tensor to add to"):
        median_hit_adjoint(cpu, g, pos, accumulate=True)
    with pytest.raises(ValueError, match="out must be a dense tensor of 10 elements"):
        median_hit_adjoint(cpu, g, pos, out=torch.zeros(10, 1))
    with pytest.raises(RuntimeError, match="there is no CPU path"):   # a state without device buffers: refused before the library
        median_hit_adjoint(cpu, g, pos)
    with pytest.raises(RuntimeError, match="grad_image is on cpu, the forward ran on cuda:0"):
        median_hit_adjoint(_state("cuda:0"), g, pos)


def test_render_prune_and_offline_take_the_switches():
    from das3r_amd import offline, prune
    from das3r_amd.render import das3r_render
    assert inspect.signature(das3r_render).parameters["return_median_depth"].default is False
    p = inspect.signature(prune.surface_scores).parameters
    assert list(p) == ["model", "views", "pipe", "background", "threshold"] and p["threshold"].default == 0.5
    assert "prune_points(model, also_drop=scores == 0)" in prune.surface_scores.__doc__
    assert inspect.signature(offline.render_sets).parameters["median_depth"].default is False
    assert inspect.signature(offline.render_set).parameters["median_depth"].default is None
    assert inspect.signature(offline.render_view_fused).parameters["median_depth"].default is False
    assert offline.parser().parse_args(["-m", "x", "-s", "y", "--median-depth"]).median_depth is True
    assert offline.parser().parse_args(["-m", "x", "-s", "y"]).median_depth is False
    z = torch.tensor([[2.0, 0.0], [1.0, 3.0]])
    assert offline.median_depth_median_rel_error(z, torch.tensor([[1.0, 5.0], [1.0, 2.0]])) == pytest.approx(0.5)
    assert offline.median_depth_median_rel_error(torch.zeros(2, 2), torch.ones(2, 2)) != offline.median_depth_median_rel_error(torch.zeros(2, 2), torch.ones(2, 2))   # NaN


def test_a_bad_threshold_stops_surface_scores_before_any_render():
    from das3r_amd import prune
    with pytest.raises(ValueError, match="threshold must be inside"):
        prune.surface_scores(object(), [], threshold=1.0)
