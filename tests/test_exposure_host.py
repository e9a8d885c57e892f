"""CPU tests of per-frame exposure compensation (INTEGRATION.md "Exposure compensation"): the library exports the three entry points under
ABI 16 and refuses bad arguments with a message; losses.apply_exposure is the transform with the index convention E[i][c]; exposure.json
round-trips; the farm's parser takes the flags; with the rates set, OptimParams / training_setup / capture_extras / restore carry the
parameter and its group (torch.optim.Adam here; FusedAdam takes the same groups), and with the defaults none of them gains anything; the
rates go into the checkpoint's loop state and a resume with others is refused; the held-out policies pick the right matrix."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

SYMBOLS = ("das3r_photometric_forward_exposure", "das3r_photometric_backward_finish_exposure", "das3r_exposure_grad_finish")
GROUPS = ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "conf_static"]


def _host_model(frames=4, H=6, W=8, seed=0, sh_degree=1):
    """tests/test_prune_host.py's CPU model: a SplatModel as create_from_frames leaves it, without its k-NN (which has no CPU path)."""
    from das3r_amd.losses import inverse_sigmoid
    from das3r_amd.model import SplatModel
    from torch import nn
    g = torch.Generator().manual_seed(seed)
    m = SplatModel(sh_degree)
    m.aggregated_mask = torch.rand(frames * H * W, generator=g) > 0.2
    P = int(m.aggregated_mask.sum())
    r = lambda *s: torch.randn(*s, generator=g)
    m._xyz = nn.Parameter(r(P, 3))
    m._features_dc = nn.Parameter(r(P, 1, 3))
    m._features_rest = nn.Parameter(0.1 * r(P, (sh_degree + 1) ** 2 - 1, 3))
    m._scaling = nn.Parameter(-2.0 + 0.3 * r(P, 3))
    m._rotation = nn.Parameter(torch.nn.functional.normalize(r(P, 4)))
    m._opacity = nn.Parameter(inverse_sigmoid(0.02 + 0.9 * torch.rand(P, 1, generator=g)))
    m._conf_static = nn.Parameter(torch.rand(frames, H, W, generator=g))
    m.Q = nn.Parameter(torch.tensor([[1.0, 0, 0, 0]]).repeat(frames, 1))
    m.T = nn.Parameter(torch.zeros(frames, 3))
    return m


def test_library_exports_the_exposure_entry_points_under_abi_16(hip_lib):
    from das3r_amd import _lib
    assert set(SYMBOLS) <= set(_lib.EXPORTS)
    assert all(hasattr(hip_lib, s) for s in SYMBOLS)
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    L = _lib.load()
    assert all(getattr(L, s).restype is C.c_int and getattr(L, s).argtypes for s in SYMBOLS), "bound in _lib"


def test_bad_arguments_are_refused_with_a_message_and_nothing_is_launched(hip_lib):
    """No device here: a call that got as far as a launch would fail otherwise.  A NULL exposure is a bad argument of its own — the existing
    symbols are the form without."""
    from das3r_amd import _lib
    L = _lib.load()
    lam = C.c_float(0.2)
    buf = (C.c_float * 16)()   # any non-NULL host address: the argument checks come before anything is touched
    p = C.cast(buf, C.c_void_p)
    assert L.das3r_photometric_forward_exposure(0, 16, p, p, p, lam, p, p, p, None) == -1
    assert b"das3r_photometric_forward_exposure" in L.das3r_last_error()
    assert L.das3r_photometric_forward_exposure(16, 16, p, p, p, lam, p, None, p, None) == -1
    assert L.das3r_photometric_forward_exposure(16, 16, p, p, p, lam, None, p, p, None) == -1
    assert b"exposure is NULL" in L.das3r_last_error()
    args = [p, p, p, lam, p, p, p, p, p, p, p, p]
    assert L.das3r_photometric_backward_finish_exposure(16, -1, *args, None) == -1
    assert b"das3r_photometric_backward_finish_exposure" in L.das3r_last_error()
    no_expo = list(args)
    no_expo[4] = None
    assert L.das3r_photometric_backward_finish_exposure(16, 16, *no_expo, None) == -1 and b"exposure is NULL" in L.das3r_last_error()
    half = list(args)
    half[9] = None   # partials without out8
    assert L.das3r_photometric_backward_finish_exposure(16, 16, *half, None) == -1 and b"go together" in L.das3r_last_error()
    no_grad = list(args)
    no_grad[7] = None   # d_render
    assert L.das3r_photometric_backward_finish_exposure(16, 16, *no_grad, None) == -1
    assert L.das3r_exposure_grad_finish(16, 16, None, p, None, None) == -1 and b"das3r_exposure_grad_finish" in L.das3r_last_error()
    assert L.das3r_exposure_grad_finish(16, 16, p, None, None, None) == -1
    assert L.das3r_exposure_grad_finish(16, 0, p, p, None, None) == -1


def test_apply_exposure_identity_returns_its_input_exactly():
    from das3r_amd.losses import apply_exposure
    g = torch.Generator().manual_seed(1)
    img = torch.rand(3, 7, 9, generator=g)
    out = apply_exposure(img, torch.eye(3, 4))
    assert out.shape == img.shape and out.dtype == img.dtype and torch.equal(out, img)
    out64 = apply_exposure(img.double(), torch.eye(3, 4))
    assert out64.dtype == torch.float64 and torch.equal(out64, img.double())


def test_apply_exposure_index_convention_on_a_hand_written_image():
    """comp_c = sum_i r_i E[i][c] + E[c][3] on a 1 x 2 image with a non-symmetric matrix, values computed by hand — E[i][c], not its
    transpose — and equal to upstream's matmul statement."""
    from das3r_amd.losses import apply_exposure
    E = torch.tensor([[1.0, 2.0, 3.0, 0.5],
                      [4.0, 5.0, 6.0, -1.0],
                      [7.0, 8.0, 10.0, 0.25]], dtype=torch.float64)
    img = torch.tensor([[[1.0, 0.0]], [[2.0, 1.0]], [[3.0, -1.0]]], dtype=torch.float64)   # pixel 0 = (1, 2, 3), pixel 1 = (0, 1, -1)
    # pixel 0: c0 = 1*1 + 2*4 + 3*7 + 0.5 = 30.5; c1 = 1*2 + 2*5 + 3*8 - 1 = 35; c2 = 1*3 + 2*6 + 3*10 + 0.25 = 45.25
    # pixel 1: c0 = 4 - 7 + 0.5 = -2.5;           c1 = 5 - 8 - 1 = -4;           c2 = 6 - 10 + 0.25 = -3.75
    want = torch.tensor([[[30.5, -2.5]], [[35.0, -4.0]], [[45.25, -3.75]]], dtype=torch.float64)
    got = apply_exposure(img, E)
    assert torch.equal(got, want), got
    transposed = apply_exposure(img, torch.cat([E[:, :3].t(), E[:, 3:]], 1))
    assert not torch.equal(transposed, want)
    upstream = torch.matmul(img.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
    assert torch.equal(got, upstream)
    # differentiable in both
    Eg, ig = E.clone().requires_grad_(True), img.clone().requires_grad_(True)
    apply_exposure(ig, Eg).sum().backward()
    assert torch.equal(Eg.grad[:, 3], torch.full((3,), 2.0, dtype=torch.float64))                 # d/dE[c][3] = number of pixels
    assert torch.equal(Eg.grad[:, 0], img.reshape(3, -1).sum(1)) and torch.equal(ig.grad[0, 0], E[0, :3].sum().expand(2))


def test_exposure_json_round_trips(tmp_path):
    import json
    from das3r_amd.io_formats import read_exposure_json, sequence_frame_names, write_exposure_json
    g = torch.Generator().manual_seed(2)
    E = torch.eye(3, 4)[None].repeat(3, 1, 1) + 0.1 * torch.randn(3, 3, 4, generator=g)
    names = ["frame_0000.png", "frame_0001.png", "frame_0003.png"]
    path = str(tmp_path / "seq" / "exposure.json")
    write_exposure_json(path, names, E)
    raw = json.load(open(path))
    assert list(raw) == names and np.asarray(raw[names[1]]).shape == (3, 4), "a dict from frame name to nested lists (upstream's file)"
    back = read_exposure_json(path)
    assert list(back) == names
    for n, m in zip(names, E):
        assert back[n].dtype == np.float32 and np.array_equal(back[n], m.numpy()), n
    assert not os.path.exists(path + ".tmp")
    with pytest.raises(ValueError):
        write_exposure_json(path, names[:2], E)
    with pytest.raises(ValueError):
        write_exposure_json(path, ["a", "a", "b"], E)
    assert sequence_frame_names(dict(images=torch.zeros(2, 3, 4, 4))) == ["frame_0000.png", "frame_0001.png"]
    assert sequence_frame_names(dict(images=torch.zeros(2, 3, 4, 4), names=["x.png", "y.png"])) == ["x.png", "y.png"]


def test_farm_and_offline_parsers_take_the_flags():
    from das3r_amd import farm, offline
    d = farm.parser().parse_args([])
    assert (d.exposure_lr_init, d.exposure_lr_final, d.exposure_heldout) == (0.0, 0.0, "identity")
    a = farm.parser().parse_args(["--exposure-lr-init", "0.01", "--exposure-lr-final", "0.001", "--exposure-heldout", "nearest"])
    assert farm.exposure_kwargs(a) == dict(exposure_lr_init=0.01, exposure_lr_final=0.001, exposure_heldout="nearest")
    with pytest.raises(SystemExit):
        farm.parser().parse_args(["--exposure-heldout", "mean"])
    o = offline.parser().parse_args(["-m", "x", "-s", "y"])
    assert o.exposure == "none"
    assert offline.parser().parse_args(["-m", "x", "-s", "y", "--exposure", "train"]).exposure == "train"


def test_switched_on_the_model_carries_the_parameter_and_its_group():
    from das3r_amd.model import OptimParams, SplatModel
    model = _host_model()
    opt = OptimParams(iterations=100, exposure_lr_init=0.01, exposure_lr_final=0.001)
    model.training_setup(opt)
    E = model._exposure
    assert isinstance(E, torch.nn.Parameter) and tuple(E.shape) == (4, 3, 4) and E.requires_grad
    assert torch.equal(E.detach(), torch.eye(3, 4)[None].repeat(4, 1, 1)), "starts as [I | 0]"
    groups = model.optimizer.param_groups
    assert [g["name"] for g in groups] == GROUPS + ["exposure"] and groups[7]["params"][0] is E and groups[7]["eps"] == 1e-15
    # the schedule: expon_lr_func(init, final, max_steps = iterations), no delay
    model.update_learning_rate(0)
    assert groups[7]["lr"] == pytest.approx(0.01, rel=1e-12)
    model.update_learning_rate(50)
    assert groups[7]["lr"] == pytest.approx((0.01 * 0.001) ** 0.5, rel=1e-9)
    model.update_learning_rate(100)
    assert groups[7]["lr"] == pytest.approx(0.001, rel=1e-9)
    # dense Adam over the whole tensor: a gradient in one row moves that row now and by momentum afterwards
    model.update_learning_rate(1)
    grad = torch.zeros_like(E)
    grad[2] = 1.0
    E.grad = grad
    model.optimizer.step()
    E.grad = torch.zeros_like(E)
    model.optimizer.step()
    assert torch.equal(E.detach()[0], torch.eye(3, 4)) and float((E.detach()[2] - torch.eye(3, 4)).abs().min()) > 0.015
    # capture_extras / restore carry it; the moments travel in the optimizer's state dict
    extras = model.capture_extras()
    assert extras["exposure"] is E
    capture = model.capture()
    other = SplatModel(1).restore(capture, opt, extras=extras)
    assert other._exposure is not E and torch.equal(other._exposure.detach(), E.detach())
    assert [g["name"] for g in other.optimizer.param_groups] == GROUPS + ["exposure"]
    st_a, st_b = model.optimizer.state[E], other.optimizer.state[other._exposure]
    assert float(st_b["step"]) == 2.0 and torch.equal(st_a["exp_avg"], st_b["exp_avg"]) and torch.equal(st_a["exp_avg_sq"], st_b["exp_avg_sq"])
    # a checkpoint with matrices cannot be restored with the feature off
    with pytest.raises(ValueError, match="exposure"):
        SplatModel(1).restore(capture, OptimParams(iterations=100), extras=extras)
    # a half-set pair is an error, not a silent off
    with pytest.raises(ValueError, match="exposure_lr"):
        _host_model().training_setup(OptimParams(exposure_lr_init=0.01))


def test_switched_off_nothing_is_gained():
    from das3r_amd.model import OptimParams, SplatModel
    opt = OptimParams(iterations=100)
    assert (opt.exposure_lr_init, opt.exposure_lr_final) == (0.0, 0.0)
    model = _host_model()
    model.training_setup(opt)
    assert model._exposure is None
    assert [g["name"] for g in model.optimizer.param_groups] == GROUPS
    extras = model.capture_extras()
    assert "exposure" not in extras
    assert set(extras) == {"conf_static", "aggregated_mask", "optimizer_cam", "test_Q", "test_T", "FoVx", "FoVy", "max_sh_degree"}
    other = SplatModel(1).restore(model.capture(), opt, extras=extras)
    assert other._exposure is None and [g["name"] for g in other.optimizer.param_groups] == GROUPS
    # switching it off again on a model that had it drops the parameter
    model.training_setup(OptimParams(iterations=100, exposure_lr_init=0.01, exposure_lr_final=0.001))
    assert model._exposure is not None
    model.training_setup(opt)
    assert model._exposure is None


def test_prune_points_leaves_the_exposure_group_alone():
    from das3r_amd.model import OptimParams
    from das3r_amd.prune import prune_points
    model = _host_model()
    model.training_setup(OptimParams(iterations=100, exposure_lr_init=0.01, exposure_lr_final=0.001))
    g = torch.Generator().manual_seed(3)
    for p in [q for gr in model.optimizer.param_groups for q in gr["params"]]:
        p.grad = torch.randn(p.shape, generator=g)
    model.update_learning_rate(1)
    model.optimizer.step()
    model.optimizer.zero_grad(set_to_none=True)
    E = model._exposure
    before = E.detach().clone()
    moments = {k: v.clone() for k, v in model.optimizer.state[E].items() if torch.is_tensor(v)}
    also = torch.zeros(model._xyz.shape[0], dtype=torch.bool)
    also[::3] = True
    info = prune_points(model, min_opacity=0.005, also_drop=also)
    assert info["dropped"] > 0
    assert model._exposure is E and torch.equal(E.detach(), before) and model.optimizer.param_groups[7]["params"][0] is E
    for k, v in moments.items():
        assert torch.equal(model.optimizer.state[E][k], v), k


def test_rates_are_kept_in_the_loop_state_and_other_rates_are_refused():
    """train() compares the loop state's rates with the OptimParams' before anything else happens (no device needed for the refusal)."""
    from das3r_amd.model import OptimParams
    from das3r_amd.train import ResumeMismatch, exposure_rates, train
    assert exposure_rates(OptimParams()) == (0.0, 0.0)
    assert exposure_rates(OptimParams(exposure_lr_init=0.01, exposure_lr_final=0.001)) == (0.01, 0.001)
    model = _host_model()
    on = OptimParams(iterations=10, exposure_lr_init=0.01, exposure_lr_final=0.001)
    model.training_setup(on)
    state = dict(exposure=(0.01, 0.001), depth_l1=(0.0, 0.0), prune=None)
    with pytest.raises(ResumeMismatch, match="exposure-lr"):
        train(model, [], OptimParams(iterations=10, exposure_lr_init=0.01, exposure_lr_final=0.01), 10, loop_state=state, start_iteration=5)
    with pytest.raises(ResumeMismatch, match="exposure-lr"):
        train(model, [], OptimParams(iterations=10), 10, loop_state=state, start_iteration=5)
    with pytest.raises(ResumeMismatch, match="exposure-lr"):   # a checkpoint from before the feature (no entry): off
        train(model, [], on, 10, loop_state=dict(depth_l1=(0.0, 0.0), prune=None), start_iteration=5)


def test_heldout_policies_pick_the_matrix_of_the_nearest_training_frame():
    from types import SimpleNamespace
    from das3r_amd.model import OptimParams
    from das3r_amd.train import heldout_exposure
    model = _host_model(frames=4)
    cam = SimpleNamespace(uid=0, frame_index=5)
    model.training_setup(OptimParams(iterations=10))
    model.exposure_frames = [0, 4, 6, 9]
    assert heldout_exposure(model, cam, "identity") is None and heldout_exposure(model, cam, "nearest") is None   # (off: no matrices)
    model.training_setup(OptimParams(iterations=10, exposure_lr_init=0.01, exposure_lr_final=0.001))
    with torch.no_grad():
        model._exposure += torch.arange(4.0).view(4, 1, 1)
    assert heldout_exposure(model, cam, "identity") is None
    E = heldout_exposure(model, cam, "nearest")
    assert torch.equal(E, model._exposure.detach()[1]) and not E.requires_grad, "frames 4 and 6 tie: the earlier one"
    assert torch.equal(heldout_exposure(model, SimpleNamespace(uid=1, frame_index=15), "nearest"), model._exposure.detach()[3])
    with pytest.raises(ValueError, match="policy"):
        heldout_exposure(model, cam, "mean")
    with pytest.raises(ValueError, match="frame_index"):
        heldout_exposure(model, SimpleNamespace(uid=0), "nearest")


def test_apply_flicker_is_affine_leaves_heldout_frames_and_returns_what_it_applied():
    from das3r_amd.train import apply_flicker, split_sequence
    g = torch.Generator().manual_seed(4)
    images = torch.rand(12, 3, 5, 7, generator=g)
    images[0, :, 0, 0], images[1, :, 0, 0] = 1.0, 0.0   # the ends of the range stay inside it
    seq = dict(images=images.clone())
    applied = apply_flicker(seq, seed=3)
    tr, te = split_sequence(seq)
    assert te == [5] and tuple(applied.shape) == (12, 3, 4)
    assert torch.equal(seq["images"][5], images[5]) and torch.equal(applied[5], torch.eye(3, 4)), "held-out frames untouched"
    for i in tr:
        gains, bias = torch.diagonal(applied[i, :, :3]), applied[i, :, 3]
        assert torch.equal(applied[i, :, :3], torch.diag(gains)), "a gain per channel, no mixing"
        assert bool((gains >= 0.7).all() and (gains <= 0.95).all() and (bias >= 0).all() and (bias <= 0.05).all())
        assert torch.allclose(seq["images"][i], images[i] * gains.view(3, 1, 1) + bias.view(3, 1, 1), rtol=0, atol=1e-7)
    assert float(seq["images"].min()) >= 0.0 and float(seq["images"].max()) <= 1.0
    assert len({float(applied[i, 0, 0]) for i in tr}) == len(tr), "every frame draws its own gains"
    again = dict(images=images.clone())
    assert torch.equal(apply_flicker(again, seed=3), applied) and torch.equal(again["images"], seq["images"]), "a seed reproduces itself"
    assert not torch.equal(apply_flicker(dict(images=images.clone()), seed=4), applied)
    with pytest.raises(AssertionError):
        apply_flicker(dict(images=images * 1.5), seed=0)
