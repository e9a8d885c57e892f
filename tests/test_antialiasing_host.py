"""CPU tests of the antialiasing mode's host plumbing (das3r_raster_saved.flags bit 4): the flag the drop-in rasterizer hands
das3r_raster_forward, the `pipe.antialiasing` das3r_render passes on, and the command lines that put --antialiasing into their pipe."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_render.npz")


def test_antialias_flag_is_bit_4_and_leaves_the_others_alone():
    from das3r_amd import _lib
    assert _lib.ANTIALIAS_FLAG == 16
    assert _lib.ANTIALIAS_FLAG & (_lib.NO_BACKWARD_IN_FLAG | 1 | 2 | 4 | 0xFF00) == 0


class _LibRecorder:
    """Stands in for the loaded library: records das3r_raster_forward's incoming flags and answers as a forward would."""

    def __init__(self):
        self.flags_in = []

    def das3r_raster_forward(self, a, i, o, ag, ab, ai, user, saved, stream):
        s = saved._obj
        self.flags_in.append(int(s.flags))
        s.flags = int(s.flags) & 16   # (the library sets bit 4 again on the way out)
        s.capacity = 0
        return 0


@pytest.fixture
def recorder(monkeypatch):
    from das3r_amd import _lib, rasterizer
    rec = _LibRecorder()
    real_empty = torch.empty

    class _Alloc:
        fns = {"geom": None, "binning": None, "img": None}

        def take(self):
            return {}

    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(rasterizer, "_fill_args", lambda rs, P, M, device, keep: _lib.RasterArgs())
    monkeypatch.setattr(rasterizer, "_fill_in", lambda *a, **k: _lib.RasterIn())
    monkeypatch.setattr(rasterizer._Alloc, "get", classmethod(lambda cls, device: _Alloc()))
    monkeypatch.setattr(rasterizer, "_on_device", lambda device: _Null())
    monkeypatch.setattr(rasterizer, "_stream", lambda device: None)
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: real_empty(*a, **k))   # (no device here: host memory)
    return rec


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class _FakeMeans:
    """means3D as _forward_full sees it on a device: [P, 3] on 'cuda'."""
    device = torch.device("cuda", 0)
    shape = (5, 3)

    def dim(self):
        return 2


def _call(**kw):
    from das3r_amd import rasterizer
    e = torch.empty(0)
    rs = SimpleNamespace(image_height=8, image_width=8)
    return rasterizer._forward_full(rs, _FakeMeans(), e, e, e, e, e, e, **kw)


def test_forward_full_enters_the_forward_with_bit_4(recorder):
    from das3r_amd import _lib
    _call()
    _call(antialiasing=True)
    _call(antialiasing=True, no_backward=True)
    _call(no_backward=True)
    assert recorder.flags_in == [0, _lib.ANTIALIAS_FLAG, _lib.ANTIALIAS_FLAG | _lib.NO_BACKWARD_IN_FLAG, _lib.NO_BACKWARD_IN_FLAG]
    cap = _call(antialiasing=True)[6]
    assert cap.flags & _lib.ANTIALIAS_FLAG   # (what _backward_impl hands back to das3r_raster_backward)


def test_drop_in_surface_has_antialiasing():
    import inspect
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer
    sig = inspect.signature(GaussianRasterizer.forward)
    assert sig.parameters["antialiasing"].default is False and sig.parameters["return_invdepth"].default is False
    assert len(GaussianRasterizationSettings._fields) == 12 and "antialiasing" not in GaussianRasterizationSettings._fields


class _RasterRecorder:
    calls = []

    def __init__(self, raster_settings):
        self.rs = raster_settings

    def __call__(self, **kw):
        _RasterRecorder.calls.append(kw)
        P = kw["means3D"].shape[0]
        out = (torch.zeros(3, int(self.rs.image_height), int(self.rs.image_width)), torch.ones(P, dtype=torch.int32))
        return out + (torch.zeros(1, int(self.rs.image_height), int(self.rs.image_width)),) if kw.get("return_invdepth") else out


def _model_and_camera():
    from das3r_amd.model import SplatModel
    gold = np.load(GOLD)
    pre = "render0_"
    pc = SplatModel(3)
    pc.active_sh_degree = int(gold[pre + "mode"][0])
    for name in ("_xyz", "_rotation", "_scaling", "_opacity", "_features_dc", "_features_rest", "_conf_static"):
        setattr(pc, name, torch.from_numpy(gold[pre + "pc" + name]).requires_grad_(True))
    pc.aggregated_mask = torch.from_numpy(gold[pre + "pc_mask"])
    fovx, fovy, H, W = gold[pre + "cam"]
    cam = SimpleNamespace(FoVx=float(fovx), FoVy=float(fovy), image_height=int(H), image_width=int(W),
                          projection_matrix=torch.from_numpy(gold[pre + "cam_proj"]), camera_center=torch.from_numpy(gold[pre + "cam_center"]),
                          world_view_transform=torch.eye(4), full_proj_transform=torch.from_numpy(gold[pre + "cam_proj"]))
    return pc, cam, torch.from_numpy(gold[pre + "bg"]), torch.from_numpy(gold[pre + "pose"])


@pytest.mark.parametrize("aa", [None, False, True])
def test_das3r_render_passes_pipe_antialiasing_through(aa, monkeypatch):
    import das3r_amd.render as R
    monkeypatch.setattr(R, "GaussianRasterizer", lambda raster_settings: _RasterRecorder(raster_settings))
    pc, cam, bg, pose = _model_and_camera()
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    if aa is not None:
        pipe.antialiasing = aa
    for fn, kw in ((R.das3r_render, dict(camera_pose=pose)), (R.das3r_render, dict(camera_pose=pose, return_invdepth=True)),
                   (R.das3r_render_3dgs, {})):
        _RasterRecorder.calls.clear()
        fn(cam, pc, pipe, bg, **kw)
        (call,) = _RasterRecorder.calls
        if aa:
            assert call.get("antialiasing") is True
        else:
            assert "antialiasing" not in call   # (upstream's call when the mode is off)
        assert call.get("return_invdepth", False) == kw.get("return_invdepth", False)


def test_farm_command_line_puts_antialiasing_into_its_pipe():
    from das3r_amd import farm
    assert farm.job_pipe(farm.parser().parse_args(["--antialiasing"])).antialiasing is True
    p = farm.job_pipe(farm.parser().parse_args([]))
    assert p.antialiasing is False and not p.debug and not p.compute_cov3D_python and not p.convert_SHs_python


def test_offline_command_line_puts_antialiasing_into_its_pipe(monkeypatch):
    from das3r_amd import io_formats, offline
    assert offline.pipe_from_args(offline.parser().parse_args(["-m", "x", "-s", "y", "--antialiasing"])).antialiasing is True
    assert offline.pipe_from_args(offline.parser().parse_args(["-m", "x", "-s", "y"])).antialiasing is False
    seen = {}
    monkeypatch.setattr(io_formats, "load_sequence", lambda *a, **k: {"depths": None})
    monkeypatch.setattr(offline, "render_sets", lambda *a, **k: (seen.update(k), (7, []))[1])
    offline.main(["-m", "x", "-s", "y", "--antialiasing", "--fused"])
    assert seen["pipe"].antialiasing is True and seen["fused"] is True

