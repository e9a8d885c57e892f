"""CPU tests of depth-supervised training's host side (INTEGRATION.md "Depth supervision"): the two additive C-ABI symbols and their
argument checks, the plain-torch statement of the loss, the weight schedule and its switches, and what a camera carries."""
import ctypes

import pytest
import torch


def test_library_exports_the_depth_l1_entry_points_under_abi_16(hip_lib):
    from das3r_amd import _lib
    assert hasattr(hip_lib, "das3r_depth_l1") and hasattr(hip_lib, "das3r_depth_l1_blocks")
    assert {"das3r_depth_l1", "das3r_depth_l1_blocks"} <= set(_lib.EXPORTS)
    assert hip_lib.das3r_abi_version() == 16, "the new entry points are additive symbols: the ABI version stays"
    assert hip_lib.das3r_depth_l1_blocks(208, 512) == (208 * 512 + 1023) // 1024
    assert hip_lib.das3r_depth_l1_blocks(1, 1) == 1 and hip_lib.das3r_depth_l1_blocks(0, 512) == 0 and hip_lib.das3r_depth_l1_blocks(16, -1) == 0


def test_depth_l1_refuses_bad_arguments_before_the_device(hip_lib):
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: the call must stop at the argument checks
    one = ctypes.c_float(1.0)
    rc = hip_lib.das3r_depth_l1(0, 32, fake, fake, fake, None, one, None, fake, fake, fake, None)
    assert rc == -1 and b"das3r_depth_l1" in hip_lib.das3r_last_error()
    rc = hip_lib.das3r_depth_l1(16, 32, None, fake, fake, None, one, None, fake, fake, fake, None)
    assert rc == -1 and b"das3r_depth_l1" in hip_lib.das3r_last_error()
    for hole in range(6):   # every required pointer: invdepth, target, mask, d_invdepth, partials, out8
        ptrs = [fake] * 6
        ptrs[hole] = None
        assert hip_lib.das3r_depth_l1(16, 32, ptrs[0], ptrs[1], ptrs[2], None, one, None, ptrs[3], ptrs[4], ptrs[5], None) == -1, hole
    assert hip_lib.das3r_depth_l1(16, -4, fake, fake, fake, None, one, None, fake, fake, fake, None) == -1
    assert hip_lib.das3r_depth_l1(1 << 16, 1 << 16, fake, fake, fake, None, one, None, fake, fake, fake, None) == -1   # (H * W does not fit)


def _maps(H, W, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    D = (0.1 + torch.rand(H, W, generator=g)).to(dtype)
    T = (0.1 + torch.rand(H, W, generator=g)).to(dtype)
    m = (torch.rand(H, W, generator=g) > 0.3).to(dtype)
    s = torch.rand(H, W, generator=g).to(dtype)
    s[torch.rand(H, W, generator=g) < 0.2] = 0.0
    return D, T, m, s


@pytest.mark.parametrize("with_static", [False, True])
def test_depth_l1_is_the_formula_written_out(with_static):
    from das3r_amd.losses import depth_l1
    H, W = 13, 21
    D, T, m, s = _maps(H, W, 1)
    if not with_static:
        s = None
    D.requires_grad_(True)
    got = depth_l1(D, T, m, s)
    total = 0.0
    for y in range(H):
        for x in range(W):
            ms = float(m[y, x]) * (float(s[y, x]) if s is not None else 1.0)
            total += abs((float(D.detach()[y, x]) - float(T[y, x])) * ms)
    assert abs(float(got) - total / (H * W)) <= 1e-14
    got.backward()
    ms = m if s is None else m * s
    closed = ms * torch.sign((D.detach() - T) * ms) / (H * W)
    assert torch.allclose(D.grad, closed, rtol=1e-14, atol=0.0)
    assert got.dtype == torch.float64
    assert depth_l1(D.detach().float()[None], T.float(), m.float(), None if s is None else s.float()).dtype == torch.float32   # ([1, H, W], any dtype)


def test_depth_l1_masked_pixels_give_exact_zeros_even_with_nan_targets():
    from das3r_amd.losses import depth_l1
    D, T, m, s = _maps(9, 14, 2)
    off = (m * s) == 0
    assert bool(off.any()) and not bool(off.all())
    clean = T.clone()
    T[off] = float("nan")
    s.requires_grad_(True)   # (the static mask is a constant of this term: nothing reaches it)
    D.requires_grad_(True)
    loss = depth_l1(D, T, m, s)
    assert torch.isfinite(loss) and float(loss) == float(depth_l1(D.detach(), clean, m, s.detach()))
    loss.backward()
    assert s.grad is None
    assert torch.isfinite(D.grad).all() and bool((D.grad[off] == 0).all()) and bool((D.grad[~off] != 0).all())
    assert float(depth_l1(D.detach(), T, torch.zeros_like(m), None)) == 0.0
    # |x| at 0: gradient 0 (torch's convention)
    E = T.clone()
    E[off] = 0.0
    E.requires_grad_(True)
    depth_l1(E, E.detach().clone(), m, None).backward()
    assert bool((E.grad == 0).all())


def test_switches_default_to_off_and_the_schedule_is_the_golden_pinned_one():
    from das3r_amd.losses import depth_l1_weight, expon_lr_func
    from das3r_amd.model import OptimParams
    opt = OptimParams()
    assert opt.depth_l1_weight_init == 0.0 and opt.depth_l1_weight_final == 0.0
    assert all(depth_l1_weight(opt, it) == 0.0 for it in (1, 2000, 4000))
    opt = OptimParams(iterations=300, depth_l1_weight_init=1.0, depth_l1_weight_final=0.01)
    f = expon_lr_func(1.0, 0.01, max_steps=300)
    for it in (1, 150, 300):
        assert depth_l1_weight(opt, it) == float(f(it)) and isinstance(depth_l1_weight(opt, it), float)
    assert abs(depth_l1_weight(opt, 150) - 0.1) < 1e-12 and abs(depth_l1_weight(opt, 300) - 0.01) < 1e-15
    with pytest.raises(ValueError):
        depth_l1_weight(OptimParams(depth_l1_weight_init=1.0), 1)   # (one end at 0: no log-linear schedule)


def test_term_is_active_only_with_a_positive_weight_and_a_camera_that_carries_the_target():
    from types import SimpleNamespace
    from das3r_amd.model import OptimParams
    from das3r_amd.train import depth_term_weight
    bare, carrying = SimpleNamespace(uid=0), SimpleNamespace(uid=0, invdepthmap=torch.zeros(2, 2), depth_mask=torch.ones(2, 2))
    on, off = OptimParams(iterations=10, depth_l1_weight_init=0.5, depth_l1_weight_final=0.5), OptimParams(iterations=10)
    assert depth_term_weight(carrying, on, 3) == pytest.approx(0.5)
    assert depth_term_weight(bare, on, 3) == 0.0 and depth_term_weight(carrying, off, 3) == 0.0 and depth_term_weight(bare, off, 3) == 0.0


def test_farm_parser_takes_the_flags_and_defaults_to_off():
    import inspect
    from das3r_amd import farm
    a = farm.parser().parse_args([])
    assert a.depth_l1_init == 0.0 and a.depth_l1_final == 0.0
    a = farm.parser().parse_args(["--depth-l1-init", "1.0", "--depth-l1-final", "0.01"])
    assert (a.depth_l1_init, a.depth_l1_final) == (1.0, 0.01)
    p = inspect.signature(farm.run_sequence_job).parameters
    assert p["depth_l1_init"].default == 0.0 and p["depth_l1_final"].default == 0.0
    assert "1.0" in farm.parser().format_help() and "0.01" in farm.parser().format_help()   # (upstream's values are named in the help text)


def test_make_camera_builds_the_depth_target_as_defined():
    from das3r_amd.train import make_camera
    H, W = 4, 6
    d = torch.full((H, W), 2.0)
    d[0, 0], d[0, 1], d[1, 2], d[2, 3], d[3, 4] = float("nan"), float("inf"), 0.0, -1.0, -float("inf")
    d[3, 5] = 0.25
    img = torch.zeros(3, H, W)
    cam = make_camera(0, img, 10.0, W, H, torch.device("cpu"), depth=d)
    bad = torch.zeros(H, W, dtype=torch.bool)
    bad[0, 0] = bad[0, 1] = bad[1, 2] = bad[2, 3] = bad[3, 4] = True
    assert cam.invdepthmap.shape == (H, W) and cam.invdepthmap.dtype == torch.float32 and cam.depth_mask.dtype == torch.float32
    assert torch.equal(cam.depth_mask, (~bad).float())
    assert bool((cam.invdepthmap[bad] == 0).all()) and torch.isfinite(cam.invdepthmap).all()
    assert torch.equal(cam.invdepthmap[~bad], 1.0 / d[~bad]) and float(cam.invdepthmap[3, 5]) == 4.0
    plain = make_camera(0, img, 10.0, W, H, torch.device("cpu"))
    assert not hasattr(plain, "invdepthmap") and not hasattr(plain, "depth_mask")
    with pytest.raises(ValueError):
        make_camera(0, img, 10.0, W, H, torch.device("cpu"), depth=torch.ones(H, W + 1))


def test_resuming_with_other_depth_weights_is_refused_before_anything_runs():
    """train() compares the weights in the checkpoint's loop state with the job's before it touches the model."""
    from das3r_amd.model import OptimParams
    from das3r_amd.train import ResumeMismatch, train
    model = type("M", (), {"get_xyz": torch.zeros(1, 3)})()
    state = dict(depth_l1=(1.0, 0.01))
    with pytest.raises(ResumeMismatch, match="depth-l1"):
        train(model, [], OptimParams(iterations=10), 10, loop_state=state, start_iteration=5)
    with pytest.raises(ResumeMismatch):
        train(model, [], OptimParams(iterations=10, depth_l1_weight_init=1.0, depth_l1_weight_final=0.01), 10, loop_state=dict(rng=None), start_iteration=5)
