"""Host-side tests of the aux channels' geometry backward (include/das3r_raster.h das3r_raster_aux_backward / _scratch_bytes) and of its
Python surface (das3r_amd.rasterizer AuxGeometry, composite_features(geometry=), alpha_of(geometry=), GaussianRasterizer(...)(...,
aux_geometry_grad=)).  No device is needed: the arguments are refused before anything is launched.  The kernel: tests/test_gpu_aux_geometry.py."""
import ctypes as C
import inspect
import os

import pytest
import torch

INVALID = -1   # DAS3R_ERR_INVALID_ARG


def _call(hip_lib, C_=1, a="ok", i="ok", saved="ok", features="p", dL_dout="p", dL_dalpha=None, dL_dfeatures=None, grads="ok", chain=False,
          scratch=True):
    """das3r_raster_aux_backward on pointers that are never dereferenced: every call here fails first."""
    from das3r_amd import _lib
    p = C.c_void_p(64)
    args = _lib.RasterArgs()
    args.P, args.image_width, args.image_height = 10, 32, 16
    rin, sv, g = _lib.RasterIn(), _lib.RasterSaved(), _lib.RasterGrads()
    sv.num_rendered = sv.capacity = 100
    if scratch:
        g.scratch = 64
    keep = _lib.Chain()
    if chain:
        g.chain = C.pointer(keep)
    pick = lambda v: p if v == "p" else v
    return hip_lib.das3r_raster_aux_backward(C.byref(args) if a == "ok" else None, C.byref(rin) if i == "ok" else None,
                                             C.byref(sv) if saved == "ok" else None, C_, pick(features), pick(dL_dout), pick(dL_dalpha),
                                             pick(dL_dfeatures), C.byref(g) if grads == "ok" else None, None)


def test_library_exports_the_entry_points_under_abi_16(hip_lib):
    from das3r_amd import _lib
    for name in ("das3r_raster_aux_backward", "das3r_raster_aux_backward_scratch_bytes"):
        assert hasattr(hip_lib, name) and name in _lib.EXPORTS
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "das3r_raster.h")) as f:
        header = f.read()
    assert "#define DAS3R_ABI_VERSION 16" in header
    assert "int das3r_raster_aux_backward(" in header and "size_t das3r_raster_aux_backward_scratch_bytes(" in header


def test_scratch_bytes_is_monotone_and_holds_a_nine_float_row_per_instance(hip_lib):
    f = hip_lib.das3r_raster_aux_backward_scratch_bytes
    caps = [0, 1, 2, 255, 256, 257, 100000, 1 << 24, 0x7FFFFF00]
    for c in range(0, 9):
        sizes = [f(cap, c) for cap in caps]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (c, sizes)
        # the nine-float rows (as das3r_raster_backward_scratch_bytes sizes them) and, behind them, C floats per instance
        assert all(s >= hip_lib.das3r_raster_backward_scratch_bytes(cap) + 4 * c * cap for s, cap in zip(sizes, caps)), (c, sizes)
        assert all(s >= 36 * cap for s, cap in zip(sizes, caps))
    for cap in caps:
        sizes = [f(cap, c) for c in range(0, 9)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (cap, sizes)


@pytest.mark.parametrize("bad_c", [9, -1, 100])
def test_a_channel_count_outside_0_to_8_is_refused(hip_lib, bad_c):
    assert _call(hip_lib, C_=bad_c) == INVALID
    err = hip_lib.das3r_last_error()
    assert b"das3r_raster_aux_backward" in err and b"channels" in err


def test_every_listed_refusal_comes_with_a_message(hip_lib):
    err = hip_lib.das3r_last_error
    # grads->chain
    assert _call(hip_lib, chain=True) == INVALID and b"das3r_raster_aux_backward" in err() and b"chain" in err()
    # C == 0 without a coverage gradient: no loss term at all
    assert _call(hip_lib, C_=0, features=None, dL_dout=None, dL_dalpha=None) == INVALID and b"dL_dalpha" in err()
    # ... and C == 0 with somewhere to put feature gradients
    assert _call(hip_lib, C_=0, features=None, dL_dout=None, dL_dalpha="p", dL_dfeatures="p") == INVALID and b"dL_dfeatures" in err()
    # a NULL among the pointers the chosen C needs
    assert _call(hip_lib, C_=3, features=None) == INVALID and b"null" in err()
    assert _call(hip_lib, C_=3, dL_dout=None) == INVALID and b"null" in err()
    assert _call(hip_lib, C_=8, features=None, dL_dout=None, dL_dalpha="p") == INVALID and b"null" in err()
    # NULL scratch
    assert _call(hip_lib, scratch=False) == INVALID and b"scratch" in err() and b"das3r_raster_aux_backward_scratch_bytes" in err()
    assert _call(hip_lib, C_=0, features=None, dL_dout=None, dL_dalpha="p", scratch=False) == INVALID and b"scratch" in err()
    # the structures themselves
    for kw in ({"a": None}, {"i": None}, {"saved": None}, {"grads": None}):
        assert _call(hip_lib, **kw) == INVALID and b"das3r_raster_aux_backward" in err() and b"null" in err(), kw
    # what das3r_raster_backward refuses is refused here as well: inputs without means3D, gradient buffers missing
    assert _call(hip_lib) == INVALID and err() != b""


def test_rasterizer_forward_keeps_its_signature_and_the_call_takes_the_keyword():
    from das3r_amd import GaussianRasterizer
    from das3r_amd.render import das3r_render
    sig = inspect.signature(GaussianRasterizer.forward)
    assert list(sig.parameters) == ["self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp",
                                    "return_invdepth", "antialiasing", "features", "return_alpha"]
    for k, v in (("shs", None), ("colors_precomp", None), ("scales", None), ("rotations", None), ("cov3D_precomp", None), ("return_invdepth", False),
                 ("antialiasing", False), ("features", None), ("return_alpha", False)):
        assert sig.parameters[k].default is v, k
    call = inspect.signature(GaussianRasterizer.__call__).parameters
    assert call["aux_geometry_grad"].default is False and call["aux_geometry_grad"].kind is inspect.Parameter.KEYWORD_ONLY
    assert call["log_focal"].default is None
    assert inspect.signature(das3r_render).parameters["aux_geometry_grad"].default is False
    for fn in ("composite_features", "alpha_of"):
        import das3r_amd
        assert inspect.signature(getattr(das3r_amd, fn)).parameters["geometry"].default is None


def _settings(W=32, H=16):
    from das3r_amd import GaussianRasterizationSettings
    return GaussianRasterizationSettings(H, W, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)


def test_aux_geometry_grad_with_no_aux_image_is_refused_in_python(monkeypatch):
    from das3r_amd import GaussianRasterizer, rasterizer

    def never(*a, **k):
        raise AssertionError("the forward must not be reached")

    monkeypatch.setattr(rasterizer, "rasterize_gaussians", never)
    z = torch.zeros(5, 3)
    r = GaussianRasterizer(_settings())
    with pytest.raises(ValueError, match="aux_geometry_grad=True needs features= and / or return_alpha=True"):
        r(means3D=z, means2D=z, opacities=torch.zeros(5, 1), colors_precomp=z, scales=z, rotations=torch.zeros(5, 4), aux_geometry_grad=True)
    assert getattr(rasterizer._last, "aux_geometry_grad", False) is False, "the keyword does not leak into the next call"


def test_default_call_is_the_one_it_was(monkeypatch):
    """aux_geometry_grad=False: nn.Module's call, one application of the colour function, no state asked for."""
    from das3r_amd import GaussianRasterizer, rasterizer
    seen = {}

    def fake(*a, antialiasing=False, options=None):
        seen["want_state"] = options.want_state
        seen["calls"] = seen.get("calls", 0) + 1
        return torch.zeros(3, 4, 4), torch.zeros(5, dtype=torch.int32)

    monkeypatch.setattr(rasterizer, "rasterize_gaussians", fake)
    z = torch.zeros(5, 3)
    r = GaussianRasterizer(_settings(4, 4))
    out = r(means3D=z, means2D=z, opacities=torch.zeros(5, 1), colors_precomp=z, scales=z, rotations=torch.zeros(5, 4), aux_geometry_grad=False)
    assert len(out) == 2 and seen == {"want_state": False, "calls": 1} and r.state is None


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


def test_composite_features_with_geometry_refuses_what_it_cannot_take(monkeypatch):
    from das3r_amd import alpha_of, composite_features
    f = torch.zeros(10, 3)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        composite_features(_state("cpu"), f, geometry=_geometry())
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        alpha_of(_state("cpu"), geometry=_geometry())
    with pytest.raises(TypeError, match="AuxGeometry"):
        composite_features(_state("cpu"), f, geometry=object())
    with pytest.raises(TypeError, match="RasterState"):
        composite_features(object(), f, geometry=_geometry())
    st = _state("cuda:0")   # (never touched: every call below fails first)
    with pytest.raises(ValueError, match="48 x 16, the forward rendered 32 x 16"):
        composite_features(st, f, geometry=_geometry(W=48))
    with pytest.raises(ValueError, match="geometry.means3D must be the forward's own tensor \\(10 rows\\)"):
        composite_features(st, f, geometry=_geometry(means3D=torch.zeros(11, 3)))
    with pytest.raises(RuntimeError, match="geometry.means3D is on cpu, the forward ran on cuda:0"):
        composite_features(st, f, geometry=_geometry())
    # the checks behind the device checks, reached with a state whose device the tensors share
    from das3r_amd import rasterizer
    monkeypatch.setattr(rasterizer, "_needs_device", lambda state: None)
    cpu = _state("cpu")
    with pytest.raises(ValueError, match="exactly one of shs / colors_precomp"):
        composite_features(cpu, f, geometry=_geometry(shs=torch.zeros(10, 1, 3)))
    with pytest.raises(ValueError, match="exactly one of the scales \\+ rotations pair / cov3D_precomp"):
        composite_features(cpu, f, geometry=_geometry(cov3D_precomp=torch.zeros(10, 6)))
    with pytest.raises(ValueError, match="geometry.scales has 9 rows"):
        composite_features(cpu, f, geometry=_geometry(scales=torch.zeros(9, 3)))
    with pytest.raises(ValueError, match="11 rows.*10 Gaussians"):
        composite_features(cpu, torch.zeros(11, 3), geometry=_geometry())
    with pytest.raises(TypeError, match="float32"):
        composite_features(cpu, f.double(), geometry=_geometry())
