"""CPU tests of the trainable field of view (das3r_raster_backward_focal, INTEGRATION.md "Focal gradients"): the per-splat reference the GPU
tests hold the kernel to (tests/focal_reference.py, through the unchanged float64 dense oracle) against central differences of the true
field-of-view change; the -1/sin(FoV) chain to the reference's parameters; the fov.json round trip; the ABI symbols and the refusals
that need no device."""
import ctypes as C
import inspect
import json
import math

import pytest
import torch

from tests import focal_reference as fr
from tests import util


def _scene(name):
    return fr.tiny_scene(int(name[4:])) if name.startswith("tiny") else util.scene_variant(name)


@pytest.mark.parametrize("name", ["tiny41", "tiny42", "tiny43", "single"])
def test_per_splat_reference_sums_to_central_differences_of_the_true_change(name):
    """sum_i c(i) of the per-splat construction against central differences of the forward with projmatrix and tanfov rebuilt, float64,
    h = 1e-6.  Bar: 1e-7 of sum|c_i| (the scenes measure 5e-11, `single` 1e-9; a missing or wrong term leaves parts in a hundred).  The
    condition that makes the differences a reference at all — no threshold flip inside the step — is that h = 2e-6 agrees equally."""
    sc, mode = _scene(name)
    c, radii = fr.per_splat(sc, mode)
    assert int((radii > 0).sum()) >= 1
    total, scale = c.sum(0), c.abs().sum(0)
    assert float(scale.min()) > 0
    for h in (1e-6, 2e-6):
        fd = fr.central_differences(sc, mode, h)
        for axis in range(2):
            rel = abs(fd[axis] - float(total[axis])) / float(scale[axis])
            print(f"{name} h={h:g} axis {axis}: autograd {float(total[axis]):+.12e} differences {fd[axis]:+.12e} rel {rel:.3e}")
            assert rel <= 1e-7, (name, h, axis, rel)


def test_chain_to_the_field_of_view_is_minus_one_over_sine():
    """s = -log tan(FoV / 2)  =>  ds/dFoV = -1 / sin(FoV): what das3r_render's stack(-log tan(FoVx / 2), ..) sends to FoVx.grad and what the
    direct step multiplies `sums` by (das3r_amd.model.fov_grad_from_log_focal)."""
    from das3r_amd.model import fov_grad_from_log_focal, log_focal_of
    fov = torch.tensor([0.35, 0.9, 1.4, 2.6], dtype=torch.float64, requires_grad=True)
    g = torch.tensor([0.7, -1.3, 2.0, 0.1], dtype=torch.float64)
    s = -torch.log(torch.tan(0.5 * fov))
    (s * g).sum().backward()
    want = -g / torch.sin(fov.detach())
    assert torch.allclose(fov.grad, want, rtol=1e-13, atol=0)
    for k in range(4):
        assert torch.allclose(fov_grad_from_log_focal(g[k], fov.detach()[k]), want[k], rtol=1e-13, atol=0)
    fx, fy = fov.detach()[0].clone().requires_grad_(True), fov.detach()[1].clone().requires_grad_(True)
    lf = log_focal_of(fx, fy)
    assert lf.shape == (2,) and torch.allclose(lf.detach(), s.detach()[:2], rtol=1e-14, atol=0)
    (lf * g[:2]).sum().backward()
    assert torch.allclose(torch.stack([fx.grad, fy.grad]), want[:2], rtol=1e-13, atol=0)


def test_fov_json_round_trip(tmp_path):
    from das3r_amd import io_formats
    path = str(tmp_path / "seq" / "fov.json")
    rec = io_formats.write_fov_json(path, 0.91, 0.55, 64, 40, 300)
    with open(path) as f:
        raw = json.load(f)
    assert set(raw) == set(io_formats.FOV_JSON_KEYS) == {"FoVx", "FoVy", "focal_x", "focal_y", "iteration"}
    back = io_formats.read_fov_json(path)
    assert back == rec and back["FoVx"] == 0.91 and back["FoVy"] == 0.55 and back["iteration"] == 300
    assert back["focal_x"] == pytest.approx(64 / (2 * math.tan(0.455)), rel=1e-15)
    assert back["focal_y"] == pytest.approx(40 / (2 * math.tan(0.275)), rel=1e-15)
    with pytest.raises(ValueError):
        io_formats.write_fov_json(path, 0.0, 0.5, 64, 40, 1)
    del raw["FoVy"]
    with open(path, "w") as f:
        json.dump(raw, f)
    with pytest.raises(ValueError, match="FoVy"):
        io_formats.read_fov_json(path)


def _host_call(lib, P=4, sums=True, work=True, depth=False):
    """das3r_raster_backward_focal on host memory: enough for the checks that come before anything is launched."""
    from das3r_amd import _lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    a = _lib.RasterArgs()
    a.P, a.sh_degree, a.M, a.image_width, a.image_height = P, 0, 1, 32, 16
    a.tanfovx = a.tanfovy = 0.5
    a.scale_modifier = 1.0
    a.bg = a.viewmatrix = a.projmatrix = a.campos = p.value
    i = _lib.RasterIn()
    i.means3D = i.opacities = i.shs = i.scales = i.rotations = p.value
    saved, g = _lib.RasterSaved(), _lib.RasterGrads()
    return lib.das3r_raster_backward_focal(C.byref(a), C.byref(i), C.byref(saved), p, p if depth else None, C.byref(g), p if sums else None, None,
                                           p if work else None, None)


def test_abi_symbols_and_refusals(monkeypatch):
    from das3r_amd import _lib
    lib = _lib.load()
    assert "das3r_raster_backward_focal" in _lib.EXPORTS and "das3r_raster_focal_workspace_bytes" in _lib.EXPORTS
    assert lib.das3r_abi_version() == _lib.ABI_VERSION == 16   # additive: the version stays
    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib._HERE), "include", "das3r_raster.h")).read()
    assert "das3r_raster_backward_focal(" in header and "das3r_raster_focal_workspace_bytes(" in header
    # one row of two floats per workgroup of 256 splats, never nothing
    for P, rows in ((0, 1), (1, 1), (256, 1), (257, 2), (1 << 20, 4096)):
        assert lib.das3r_raster_focal_workspace_bytes(P) == 8 * rows
    INVALID = -1
    for kw in (dict(sums=False), dict(work=False), dict(sums=False, work=False, P=0)):
        assert _host_call(lib, **kw) == INVALID
        assert "das3r_raster_backward_focal: null sums / workspace" in _lib.last_error()
    # the forced forms das3r_raster_backward_depth refuses, refused here too once there is a dL_dinvdepth — before the saved state is looked at
    monkeypatch.setenv("DAS3R_RENDER_BWD", "scan128")
    _lib.reload_switches()
    try:
        assert _host_call(lib, depth=True) == INVALID
        assert "das3r_raster_backward_focal: DAS3R_RENDER_BWD=scan has no inverse-depth form" in _lib.last_error()
        # colour only: the form is not refused; the call gets as far as the (empty) saved state
        assert _host_call(lib) == INVALID
        assert "null saved state" in _lib.last_error()
    finally:
        monkeypatch.delenv("DAS3R_RENDER_BWD")
        _lib.reload_switches()
    assert _host_call(lib, depth=True) == INVALID and "null saved state" in _lib.last_error()


def test_farm_and_offline_take_the_options(tmp_path):
    """farm --fov-lr (default 0: off) reaches run_sequence_job; offline renders with <model-path>/fov.json unless --camera-fov (apply_fov: the
    cameras' field of view and the projection make_camera builds from it)."""
    from das3r_amd import farm, offline
    from das3r_amd.camera import focal2fov
    from das3r_amd.train import make_camera
    assert farm.parser().parse_args([]).fov_lr == 0.0 and farm.parser().parse_args(["--fov-lr", "2e-4"]).fov_lr == 2e-4
    assert "fov_lr" in inspect.signature(farm.run_sequence_job).parameters
    assert inspect.signature(farm.run_sequence_job).parameters["fov_lr"].default == 0.0
    a = offline.parser().parse_args(["-m", "x", "-s", "y"])
    assert a.camera_fov is False and offline.parser().parse_args(["-m", "x", "-s", "y", "--camera-fov"]).camera_fov is True
    assert inspect.signature(offline.render_sets).parameters["camera_fov"].default is False
    cams = [make_camera(i, torch.zeros(3, 40, 64), 55.0, 64, 40, "cpu") for i in range(2)]
    fx, fy = focal2fov(57.0, 64), focal2fov(56.0, 40)
    offline.apply_fov(cams, fx, fy)
    want = make_camera(0, torch.zeros(3, 40, 64), 57.0, 64, 40, "cpu", focal_y=56.0)
    for c in cams:
        assert c.FoVx == fx and c.FoVy == fy and torch.equal(c.projection_matrix, want.projection_matrix)


def test_fov_lr_sets_the_groups_and_defaults_to_the_reference(monkeypatch):
    """OptimParams.fov_lr: 0 by default — the groups stay at the reference's 1e-4 and model.fov_lr is 0 (nothing renders with the model's field
    of view); > 0 — both groups take it; negative or without a field of view on the model: refused."""
    from das3r_amd.model import OptimParams, SplatModel
    assert OptimParams().fov_lr == 0.0
    m = SplatModel(0)
    n = 6
    for name, shape in (("_xyz", (n, 3)), ("_features_dc", (n, 1, 3)), ("_features_rest", (n, 0, 3)), ("_opacity", (n, 1)), ("_scaling", (n, 3)),
                        ("_rotation", (n, 4)), ("_conf_static", (1, 2, 3)), ("Q", (1, 4)), ("T", (1, 3))):
        setattr(m, name, torch.nn.Parameter(torch.zeros(shape)))
    with pytest.raises(RuntimeError, match="init_fov"):
        m.training_setup(OptimParams(fov_lr=1e-3))
    m.init_fov(0.9, 0.6)
    m.training_setup(OptimParams())
    assert m.fov_lr == 0.0 and [g["lr"] for g in m.optimizer_cam.param_groups[2:]] == [0.0001, 0.0001]
    m.training_setup(OptimParams(fov_lr=2e-4))
    assert m.fov_lr == 2e-4 and [(g["name"], g["lr"]) for g in m.optimizer_cam.param_groups[2:]] == [("fovX", 2e-4), ("fovY", 2e-4)]
    with pytest.raises(ValueError, match="fov_lr"):
        m.training_setup(OptimParams(fov_lr=-1.0))
