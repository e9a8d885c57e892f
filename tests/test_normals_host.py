"""Host-side tests of the normal-consistency regulariser's entry points (include/das3r_raster.h das3r_gaussian_normals_forward / _backward,
das3r_normal_consistency_forward / _backward) and of its Python surface (das3r_amd.gaussian_normals / depth_normals / normal_consistency,
das3r_render(return_normals=, return_normal_consistency=, normal_depth=), OptimParams.normal_weight / normal_depth, train_step, farm,
offline).  No device is needed: the arguments are refused before anything is launched.  The kernels: tests/test_gpu_normals.py."""
import ctypes as C
import inspect
import os

import pytest
import torch

INVALID = -1   # DAS3R_ERR_INVALID_ARG
OK = 0
NAMES = ("das3r_gaussian_normals_forward", "das3r_gaussian_normals_backward", "das3r_normal_consistency_forward",
         "das3r_normal_consistency_backward")
P_ = C.c_void_p(64)   # a pointer that is never dereferenced: every call here returns before a launch


def _args(P=10, view=True, campos=True):
    from das3r_amd import _lib
    a = _lib.RasterArgs()
    a.P = P
    a.viewmatrix = 64 if view else None
    a.campos = 64 if campos else None
    return a


def test_library_exports_the_entry_points_under_abi_16(hip_lib):
    from das3r_amd import _lib
    for name in NAMES:
        assert hasattr(hip_lib, name) and name in _lib.EXPORTS
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "das3r_raster.h")) as f:
        header = f.read()
    assert "#define DAS3R_ABI_VERSION 16" in header
    for name in NAMES:
        assert f"int {name}(" in header
    # the definition is fixed there, word for word
    for text in ("k = argmin_j scales[i][j].  Ties take the lowest j.", "flip = (a . d > 0).  A dot product of exactly 0 keeps a.",
                 "choice[i] = k | (flip << 2)", "not an\n * eigenvector of the sheared covariance",
                 "t_x = 2 tanfovx / W, t_y = 2 tanfovy / H", "dx = ((z+ - z-) r_x + (z+ + z-) t_x,  (z+ - z-) r_y,  z+ - z-)", "N_d = (dy x dx) / |dy x dx|",
                 "loss = m (alpha - normal . N_d)", "dL_dalpha = g m;  dL_dnormal = -g m N_d", "GATHER form"):
        assert text in header, text


def test_the_unit_is_built_without_fma_contraction():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "das3r_amd", "csrc", "Makefile")) as f:
        rules = [line for line in f.read().splitlines() if line.endswith(": %.o: %.hip $(HDRS)")]
    exact = [r for r in rules if "preprocess.o" in r.split(":")[0].split()]
    assert len(exact) == 1 and "normals.o" in exact[0].split(":")[0].split()


def test_every_listed_refusal_of_the_gaussian_normals_comes_with_a_message(hip_lib):
    err = hip_lib.das3r_last_error
    fwd, bwd = hip_lib.das3r_gaussian_normals_forward, hip_lib.das3r_gaussian_normals_backward
    who = b"das3r_gaussian_normals_forward"
    assert fwd(None, P_, P_, P_, P_, P_, None) == INVALID and who in err() and b"null args" in err()
    assert fwd(C.byref(_args(P=-1)), P_, P_, P_, P_, P_, None) == INVALID and who in err() and b"P = -1" in err()
    assert fwd(C.byref(_args(view=False)), P_, P_, P_, P_, P_, None) == INVALID and who in err() and b"viewmatrix" in err()
    assert fwd(C.byref(_args(campos=False)), P_, P_, P_, P_, P_, None) == INVALID and who in err() and b"campos" in err()
    for hole in range(5):
        ptrs = [None if k == hole else P_ for k in range(5)]
        assert fwd(C.byref(_args()), *ptrs, None) == INVALID and who in err() and b"null" in err(), hole
    who = b"das3r_gaussian_normals_backward"
    assert bwd(None, P_, P_, P_, P_, 0, None) == INVALID and who in err() and b"null args" in err()
    assert bwd(C.byref(_args(P=-5)), P_, P_, P_, P_, 0, None) == INVALID and who in err()
    assert bwd(C.byref(_args(view=False)), P_, P_, P_, P_, 0, None) == INVALID and who in err() and b"viewmatrix" in err()
    for hole in range(4):
        ptrs = [None if k == hole else P_ for k in range(4)]
        assert bwd(C.byref(_args()), *ptrs, 1, None) == INVALID and who in err() and b"null" in err(), hole


def test_no_gaussian_is_ok_and_launches_nothing(hip_lib):
    """P == 0 returns before any pointer is looked at: with never-dereferenced pointers, and with none at all."""
    assert hip_lib.das3r_gaussian_normals_forward(C.byref(_args(P=0)), P_, P_, P_, P_, P_, None) == OK
    assert hip_lib.das3r_gaussian_normals_forward(C.byref(_args(P=0, view=False, campos=False)), None, None, None, None, None, None) == OK
    assert hip_lib.das3r_gaussian_normals_backward(C.byref(_args(P=0)), None, None, None, None, 0, None) == OK


def test_every_listed_refusal_of_the_image_entries_comes_with_a_message(hip_lib):
    err = hip_lib.das3r_last_error
    fwd, bwd = hip_lib.das3r_normal_consistency_forward, hip_lib.das3r_normal_consistency_backward
    nan, inf = float("nan"), float("inf")
    who = b"das3r_normal_consistency_forward"
    good = (P_, P_, P_, P_, P_, P_)
    for H, W in ((0, 8), (8, 0), (-1, 8), (8, -3), (1 << 15, (1 << 15) + 1), (1 << 30, 2)):
        assert fwd(H, W, 1.0, 1.0, *good, None) == INVALID and who in err() and b"extents" in err(), (H, W)
    for tx, ty in ((nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, -inf)):
        assert fwd(8, 8, tx, ty, *good, None) == INVALID and who in err() and b"finite" in err(), (tx, ty)
    for hole in (0, 1, 2, 4):   # depth, normal, alpha, loss; mask (3) and depth_normal (5) may be NULL
        ptrs = [None if k == hole else P_ for k in range(6)]
        assert fwd(8, 8, 1.0, 1.0, *ptrs, None) == INVALID and who in err() and b"null" in err(), hole
    who = b"das3r_normal_consistency_backward"
    good = (P_,) * 7
    for H, W in ((0, 8), (8, 0), (1 << 15, (1 << 15) + 1)):
        assert bwd(H, W, 1.0, 1.0, *good, None) == INVALID and who in err() and b"extents" in err(), (H, W)
    assert bwd(8, 8, nan, 1.0, *good, None) == INVALID and who in err() and b"finite" in err()
    assert bwd(8, 8, 1.0, inf, *good, None) == INVALID and who in err() and b"finite" in err()
    for hole in (0, 1, 3, 4, 5, 6):   # depth, normal, dL_dloss, dL_ddepth, dL_dnormal, dL_dalpha; mask (2) may be NULL
        ptrs = [None if k == hole else P_ for k in range(7)]
        assert bwd(8, 8, 1.0, 1.0, *ptrs, None) == INVALID and who in err() and b"null" in err(), hole


def _settings(W=32, H=16):
    from das3r_amd import GaussianRasterizationSettings
    return GaussianRasterizationSettings(H, W, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)


def test_the_python_names_are_exported():
    import das3r_amd
    from das3r_amd import rasterizer
    for name in ("gaussian_normals", "depth_normals", "normal_consistency"):
        assert getattr(das3r_amd, name) is getattr(rasterizer, name) and name in das3r_amd.__all__
    assert list(inspect.signature(das3r_amd.gaussian_normals).parameters) == ["raster_settings", "rotations", "scales", "means3D"]
    assert list(inspect.signature(das3r_amd.depth_normals).parameters) == ["depth", "raster_settings"]
    sig = inspect.signature(das3r_amd.normal_consistency)
    assert list(sig.parameters) == ["depth", "normal", "alpha", "raster_settings", "mask"] and sig.parameters["mask"].default is None


def test_the_python_side_refuses_what_it_cannot_take():
    from das3r_amd import depth_normals, gaussian_normals, normal_consistency
    rs = _settings()
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match="a cov3D_precomp caller has no axes"):
        gaussian_normals(rs, None, None, z(10, 3))
    with pytest.raises(ValueError, match="a cov3D_precomp caller has no axes"):
        gaussian_normals(rs, torch.empty(0), torch.empty(0), z(10, 3))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        gaussian_normals(rs, z(10, 4), z(10, 3), z(10, 3))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        depth_normals(z(16, 32), rs)
    with pytest.raises(ValueError, match=r"depth must have dimensions \(16, 32\) or \(1, 16, 32\)"):
        depth_normals(z(32, 16), rs)
    with pytest.raises(TypeError, match="depth must be float32"):
        depth_normals(z(16, 32).double(), rs)
    with pytest.raises(ValueError, match=r"normal must be a float32 tensor of dimensions \(3, 16, 32\)"):
        normal_consistency(z(16, 32), z(2, 16, 32), z(16, 32), rs)
    with pytest.raises(ValueError, match="alpha must have dimensions"):
        normal_consistency(z(16, 32), z(3, 16, 32), z(16, 31), rs)
    with pytest.raises(ValueError, match="mask must have dimensions"):
        normal_consistency(z(16, 32), z(3, 16, 32), z(16, 32), rs, mask=z(3, 16, 32))


def test_render_and_optimizer_parameters_default_to_off():
    from das3r_amd.model import OptimParams
    from das3r_amd.render import das3r_render
    p = inspect.signature(das3r_render).parameters
    assert p["return_normals"].default is False and p["return_normal_consistency"].default is False
    assert p["normal_depth"].default == "median" and p["normal_mask"].default is None
    assert OptimParams().normal_weight == 0.0 and isinstance(OptimParams().normal_weight, float) and OptimParams().normal_depth == "median"


def test_a_bad_normal_depth_is_refused_before_anything_is_rendered():
    from das3r_amd.render import das3r_render
    with pytest.raises(ValueError, match="normal_depth must be one of"):
        das3r_render(object(), object(), object(), None, normal_depth="mean")
    with pytest.raises(ValueError, match="normal_depth must be one of"):
        das3r_render(object(), object(), object(), None, return_normal_consistency=True, normal_depth=None)


def test_a_bad_weight_or_depth_mode_is_refused():
    from das3r_amd import train
    from das3r_amd.model import OptimParams
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="normal_weight"):
            train.normal_term_weight(OptimParams(normal_weight=bad))
    assert train.normal_term_weight(OptimParams(normal_weight=0.25)) == 0.25 and train.normal_term_weight(object()) == 0.0
    with pytest.raises(ValueError, match="normal_depth"):
        train.normal_term_depth(OptimParams(normal_depth="mean"))
    assert train.normal_term_depth(OptimParams(normal_depth="blended")) == "blended" and train.normal_term_depth(object()) == "median"


class _Stop(Exception):
    pass


def _train_step_route(monkeypatch, **opt_kw):
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

    try:
        out = train.train_step(Model(), object(), OptimParams(**opt_kw), 1, object(), None, fused=True)
        assert out == ("loss", "psnr", {})
    except _Stop:
        pass
    return seen


def test_with_the_weight_at_zero_train_step_still_reaches_the_direct_iteration(monkeypatch):
    assert _train_step_route(monkeypatch, normal_weight=0.0) == ["direct"]
    assert _train_step_route(monkeypatch, normal_weight=0.0, normal_depth="blended") == ["direct"]


def test_with_the_weight_on_train_step_takes_the_autograd_form(monkeypatch):
    assert _train_step_route(monkeypatch, normal_weight=0.5) == ["autograd"]
    with pytest.raises(ValueError, match="normal_depth"):
        _train_step_route(monkeypatch, normal_weight=0.5, normal_depth="mean")


def test_train_step_asks_the_render_for_the_term_with_the_static_map_as_mask(monkeypatch):
    """With the weight on, das3r_render is called with return_normal_consistency, the mode and the frame's static map (detached); at 0 with none
    of the three."""
    from types import SimpleNamespace
    from das3r_amd import train
    from das3r_amd.model import OptimParams
    calls = []

    def render(cam, model, pipe, bg, **kw):
        calls.append(kw)
        raise _Stop()

    monkeypatch.setattr(train, "das3r_render", render)
    static = torch.nn.Parameter(torch.rand(2, 4, 5))
    model = SimpleNamespace(update_learning_rate=lambda it: None, get_RT=lambda uid: None, _conf_static=static, oneupSHdegree=lambda: None)
    cam = SimpleNamespace(uid=1)
    for kw in ({}, {"normal_weight": 0.5, "normal_depth": "blended"}):
        with pytest.raises(_Stop):
            train.train_step(model, cam, OptimParams(**kw), 1, object(), None, fused=False)
    off, on = calls
    assert not any(k.startswith("normal") or k.startswith("return_normal") for k in off)
    assert on["return_normal_consistency"] is True and on["normal_depth"] == "blended"
    assert torch.equal(on["normal_mask"], static[1].detach()) and not on["normal_mask"].requires_grad


def test_farm_and_offline_take_the_switches():
    from das3r_amd import farm, offline
    p = inspect.signature(farm.run_sequence_job).parameters
    assert p["normal_weight"].default == 0.0 and p["normal_depth"].default == "median"
    assert inspect.signature(offline.render_sets).parameters["normals"].default is False
    assert inspect.signature(offline.render_set).parameters["normals"].default is None
    assert inspect.signature(offline.render_view_fused).parameters["normals"].default is False
    assert offline.parser().parse_args(["-m", "x", "-s", "y", "--normals"]).normals is True
    assert offline.parser().parse_args(["-m", "x", "-s", "y"]).normals is False
    opt = [a for a in farm.parser()._actions if "--normal-weight" in a.option_strings]
    assert len(opt) == 1 and opt[0].default == 0.0 and opt[0].type is float
    opt = [a for a in farm.parser()._actions if "--normal-depth" in a.option_strings]
    assert len(opt) == 1 and opt[0].default == "median" and tuple(opt[0].choices) == ("median", "blended")
