"""Host-side tests of the ray-distortion regulariser's entry points (include/das3r_raster.h das3r_raster_distortion_forward / _backward /
_backward_scratch_bytes) and of its Python surface (das3r_amd.distortion_of, das3r_render(return_distortion=), OptimParams.distortion_weight,
train_step).  No device is needed: the arguments are refused before anything is launched.  The kernels: tests/test_gpu_distortion.py."""
import ctypes as C
import inspect
import os

import pytest
import torch

INVALID = -1   # DAS3R_ERR_INVALID_ARG


def _structs(scratch=True, chain=False):
    from das3r_amd import _lib
    args = _lib.RasterArgs()
    args.P, args.image_width, args.image_height = 10, 32, 16
    rin, sv, g = _lib.RasterIn(), _lib.RasterSaved(), _lib.RasterGrads()
    sv.num_rendered = sv.capacity = 100
    if scratch:
        g.scratch = 64
    keep = _lib.Chain()
    if chain:
        g.chain = C.pointer(keep)
    return args, rin, sv, g, keep


def _backward(hip_lib, a="ok", i="ok", saved="ok", dL="p", totals="p", grads="ok", chain=False, scratch=True):
    """das3r_raster_distortion_backward on pointers that are never dereferenced: every call here fails first."""
    p = C.c_void_p(64)
    args, rin, sv, g, keep = _structs(scratch, chain)
    pick = lambda v: p if v == "p" else v
    return hip_lib.das3r_raster_distortion_backward(C.byref(args) if a == "ok" else None, C.byref(rin) if i == "ok" else None,
                                                    C.byref(sv) if saved == "ok" else None, pick(dL), pick(totals),
                                                    C.byref(g) if grads == "ok" else None, None)


def _forward(hip_lib, a="ok", saved="ok", out="p", W=32):
    p = C.c_void_p(64)
    args, _, sv, _, _ = _structs()
    args.image_width = W
    return hip_lib.das3r_raster_distortion_forward(C.byref(args) if a == "ok" else None, C.byref(sv) if saved == "ok" else None,
                                                   p if out == "p" else None, None, None)


NAMES = ("das3r_raster_distortion_forward", "das3r_raster_distortion_backward_scratch_bytes", "das3r_raster_distortion_backward")


def test_library_exports_the_entry_points_under_abi_16(hip_lib):
    from das3r_amd import _lib
    for name in NAMES:
        assert hasattr(hip_lib, name) and name in _lib.EXPORTS
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "das3r_raster.h")) as f:
        header = f.read()
    assert "#define DAS3R_ABI_VERSION 16" in header
    assert "int das3r_raster_distortion_forward(" in header and "int das3r_raster_distortion_backward(" in header
    assert "size_t das3r_raster_distortion_backward_scratch_bytes(" in header
    # the definition is fixed there: both forms, the shift, the totals-plane design and the backward formulas
    for text in ("D[pixel] = sum_{j<k} w_j w_k (m_j - m_k)", "sum_k w_k (B_{k-1} - m_k A_{k-1})", "m_k (2 SA_k - A) - (2 SB_k - B)",
                 "w_k (2 SA_k + w_k - A)", "THE TOTALS PLANE", "RELATIVE TO THE PIXEL'S WEIGHTED MEAN"):
        assert text in header, text


def test_scratch_bytes_is_monotone_and_holds_the_rows_and_a_float_per_gaussian(hip_lib):
    f = hip_lib.das3r_raster_distortion_backward_scratch_bytes
    caps = [0, 1, 2, 255, 256, 257, 100000, 1 << 24, 0x7FFFFF00]
    Ps = [0, 1, 7, 1000, 1 << 20, 0x7FFFFFFF]
    for P in Ps:
        sizes = [f(cap, P) for cap in caps]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (P, sizes)
        assert all(s >= hip_lib.das3r_raster_backward_scratch_bytes(cap) + 4 * P for s, cap in zip(sizes, caps)), (P, sizes)
        assert all(s >= 36 * cap for s, cap in zip(sizes, caps))
    for cap in caps:
        sizes = [f(cap, P) for P in Ps]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), (cap, sizes)


def test_every_listed_refusal_of_the_backward_comes_with_a_message(hip_lib):
    err = hip_lib.das3r_last_error
    who = b"das3r_raster_distortion_backward"
    for kw in ({"a": None}, {"i": None}, {"saved": None}, {"grads": None}):
        assert _backward(hip_lib, **kw) == INVALID and who in err() and b"null" in err(), kw
    assert _backward(hip_lib, dL=None) == INVALID and who in err() and b"dL_ddist" in err()
    assert _backward(hip_lib, totals=None) == INVALID and who in err() and b"totals" in err()
    assert _backward(hip_lib, scratch=False) == INVALID and who in err() and b"das3r_raster_distortion_backward_scratch_bytes" in err()
    assert _backward(hip_lib, chain=True) == INVALID and who in err() and b"chain" in err()
    # what das3r_raster_backward refuses is refused here as well: inputs without means3D, gradient buffers missing
    assert _backward(hip_lib) == INVALID and err() != b""


def test_every_listed_refusal_of_the_forward_comes_with_a_message(hip_lib):
    err = hip_lib.das3r_last_error
    who = b"das3r_raster_distortion_forward"
    for kw in ({"a": None}, {"saved": None}, {"out": None}):
        assert _forward(hip_lib, **kw) == INVALID and who in err() and b"null" in err(), kw
    assert _forward(hip_lib, W=0) == INVALID and who in err() and b"extents" in err()
    assert _forward(hip_lib) == INVALID and who in err() and b"saved buffers missing" in err()


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


def test_distortion_of_is_exported_beside_alpha_of():
    import das3r_amd
    from das3r_amd import rasterizer
    assert das3r_amd.distortion_of is rasterizer.distortion_of and "distortion_of" in das3r_amd.__all__
    sig = inspect.signature(das3r_amd.distortion_of)
    assert list(sig.parameters) == ["state", "geometry"] and sig.parameters["geometry"].default is None


def test_distortion_of_refuses_what_it_cannot_take(monkeypatch):
    from das3r_amd import distortion_of, rasterizer
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        distortion_of(_state("cpu"))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        distortion_of(_state("cpu"), geometry=_geometry())
    with pytest.raises(TypeError, match="AuxGeometry"):
        distortion_of(_state("cpu"), geometry=object())
    with pytest.raises(TypeError, match="RasterState"):
        distortion_of(object())
    with pytest.raises(TypeError, match="RasterState"):
        distortion_of(object(), geometry=_geometry())
    st = _state("cuda:0")   # (never touched: every call below fails first)
    with pytest.raises(ValueError, match="48 x 16, the forward rendered 32 x 16"):
        distortion_of(st, geometry=_geometry(W=48))
    with pytest.raises(ValueError, match="geometry.means3D must be the forward's own tensor \\(10 rows\\)"):
        distortion_of(st, geometry=_geometry(means3D=torch.zeros(11, 3)))
    with pytest.raises(RuntimeError, match="geometry.means3D is on cpu, the forward ran on cuda:0"):
        distortion_of(st, geometry=_geometry())
    monkeypatch.setattr(rasterizer, "_needs_device", lambda state: None)
    cpu = _state("cpu")
    with pytest.raises(ValueError, match="exactly one of shs / colors_precomp"):
        distortion_of(cpu, geometry=_geometry(shs=torch.zeros(10, 1, 3)))
    with pytest.raises(ValueError, match="exactly one of the scales \\+ rotations pair / cov3D_precomp"):
        distortion_of(cpu, geometry=_geometry(cov3D_precomp=torch.zeros(10, 6)))
    with pytest.raises(ValueError, match="geometry.scales has 9 rows"):
        distortion_of(cpu, geometry=_geometry(scales=torch.zeros(9, 3)))


def test_render_and_optimizer_parameters_default_to_off():
    from das3r_amd.model import OptimParams
    from das3r_amd.render import das3r_render
    p = inspect.signature(das3r_render).parameters["return_distortion"]
    assert p.default is False
    assert OptimParams().distortion_weight == 0.0 and isinstance(OptimParams().distortion_weight, float)


class _Stop(Exception):
    pass


def _train_step_route(weight, monkeypatch):
    """-> which of (fast_step.train_step, the autograd form) train_step(fused=True) enters; both are stubbed: no device, no model."""
    from das3r_amd import fast_step, train
    from das3r_amd.model import OptimParams
    seen = []
    monkeypatch.setattr(fast_step, "available", lambda model, pipe: True)
    monkeypatch.setattr(fast_step, "train_step", lambda *a, **k: seen.append("direct") or ("loss", "psnr", {}))

    class Model:
        def update_learning_rate(self, iteration):
            seen.append("autograd")
            raise _Stop()

    opt = OptimParams(distortion_weight=weight)
    try:
        out = train.train_step(Model(), object(), opt, 1, object(), None, fused=True)
        assert out == ("loss", "psnr", {})
    except _Stop:
        pass
    return seen


def test_with_the_weight_at_zero_train_step_still_reaches_the_direct_iteration(monkeypatch):
    assert _train_step_route(0.0, monkeypatch) == ["direct"]


def test_with_the_weight_on_train_step_takes_the_autograd_form(monkeypatch):
    assert _train_step_route(0.5, monkeypatch) == ["autograd"]


def test_a_bad_weight_is_refused():
    from das3r_amd import train
    from das3r_amd.model import OptimParams
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="distortion_weight"):
            train.distortion_term_weight(OptimParams(distortion_weight=bad))


def test_farm_and_offline_take_the_switches():
    from das3r_amd import farm, offline
    assert inspect.signature(farm.run_sequence_job).parameters["distortion_weight"].default == 0.0
    assert inspect.signature(offline.render_sets).parameters["distortion"].default is False
    assert inspect.signature(offline.render_set).parameters["distortion"].default is None
    assert offline.parser().parse_args(["-m", "x", "-s", "y", "--distortion"]).distortion is True
    assert offline.parser().parse_args(["-m", "x", "-s", "y"]).distortion is False
    opt = [a for a in farm.parser()._actions if "--distortion-weight" in a.option_strings]
    assert len(opt) == 1 and opt[0].default == 0.0 and opt[0].type is float
