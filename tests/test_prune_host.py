"""CPU tests of pruning (das3r_amd/prune.py, INTEGRATION.md "Pruning"): the library exports the two entry points under ABI 16; the torch
form of the model surgery equals a direct restatement, for torch.optim.Adam and for FusedAdam's state (compact SH moments included); the
schedule is off by default, is kept in the checkpoint's loop state, and a resume with other settings is refused; restore() to another P
drops the cached pixel index."""
import copy

import pytest
import torch

PARAMS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


def _host_model(frames=3, H=10, W=14, seed=0, sh_degree=3):
    """A SplatModel on the CPU as create_from_frames leaves it (without its k-NN, which has no CPU path): some pixels are not Gaussians
    (confidence below the threshold), conf_static is per pixel."""
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
    opac = 0.02 + 0.9 * torch.rand(P, 1, generator=g)
    opac[torch.rand(P, generator=g) < 0.2] = 0.001      # learned down
    m._opacity = nn.Parameter(inverse_sigmoid(opac))
    conf = torch.rand(frames, H, W, generator=g)
    conf[torch.rand(frames, H, W, generator=g) < 0.15] = 0.0   # the moving object
    conf.view(-1)[5] = -0.25                                   # (the parameter is unclamped)
    m._conf_static = nn.Parameter(conf)
    m.Q = nn.Parameter(torch.tensor([[1.0, 0, 0, 0]]).repeat(frames, 1))
    m.T = nn.Parameter(torch.zeros(frames, 3))
    return m


def _restatement(model, min_opacity, max_world_scale=0.0, also_drop=None):
    idx = torch.nonzero(model.aggregated_mask.reshape(-1)).reshape(-1)
    eff = torch.sigmoid(model._opacity.detach()).reshape(-1) * model._conf_static.detach().reshape(-1)[idx]
    drop = eff < torch.tensor(min_opacity, dtype=torch.float32)
    if max_world_scale > 0:
        drop |= torch.exp(model._scaling.detach()).max(dim=1).values > max_world_scale
    if also_drop is not None:
        drop |= also_drop
    keep = ~drop
    mask = model.aggregated_mask.clone()
    mask[idx[drop]] = False
    return keep, mask, idx[keep]


def test_library_exports_the_prune_entry_points_under_abi_16(hip_lib):
    from das3r_amd import _lib
    assert {"das3r_prune_select", "das3r_prune_compact"} <= set(_lib.EXPORTS)
    assert hasattr(hip_lib, "das3r_prune_select") and hasattr(hip_lib, "das3r_prune_compact")
    assert hip_lib.das3r_abi_version() == 16 == _lib.ABI_VERSION
    assert _lib.prune_count_words(0) == 1 and _lib.prune_count_words(1024) == 2 and _lib.prune_count_words(1025) == 3
    # bad arguments are reported, nothing is launched (no device here)
    assert hip_lib.das3r_prune_select(-1, None, None, None, 0.5, None, 0.0, None, None, None, None) == -1
    assert hip_lib.das3r_prune_select(5, None, None, None, 0.5, None, 0.0, None, None, None, None) == -1
    t = (_lib.PruneTensor * 1)()
    assert hip_lib.das3r_prune_compact(4, 5, None, 1, t, None) == -1 and b"kept" in hip_lib.das3r_last_error()
    assert hip_lib.das3r_prune_compact(0, 0, None, 0, None, None) == 0


@pytest.mark.parametrize("max_world_scale,with_mask", [(0.0, False), (0.16, False), (0.0, True)])
def test_prune_points_on_a_host_model_with_torch_adam_equals_a_restatement(max_world_scale, with_mask):
    from das3r_amd.model import OptimParams
    from das3r_amd.prune import prune_points
    model = _host_model()
    opt = OptimParams(iterations=100)
    model.training_setup(opt)
    P = model._xyz.shape[0]
    g = torch.Generator().manual_seed(3)
    for _ in range(2):   # two real steps: moments and step counts exist
        for n in PARAMS + ("_conf_static",):
            getattr(model, n).grad = torch.randn(getattr(model, n).shape, generator=g)
        model.update_learning_rate(1)
        model.optimizer.step()
    model.optimizer.zero_grad(set_to_none=True)
    also = (torch.rand(P, generator=g) < 0.1) if with_mask else None
    keep, mask, index = _restatement(model, 0.005, max_world_scale, also)
    assert 0 < int(keep.sum()) < P
    before = {n: getattr(model, n).detach().clone() for n in PARAMS}
    old = {n: getattr(model, n) for n in PARAMS}
    moments = {n: {k: v.clone() for k, v in model.optimizer.state[old[n]].items()} for n in PARAMS}
    conf_before, cam_state = model._conf_static, model.optimizer_cam.state_dict()
    info = prune_points(model, min_opacity=0.005, max_world_scale=max_world_scale, also_drop=also)
    Pn = int(keep.sum())
    assert info == dict(before=P, after=Pn, dropped=P - Pn, path="torch")
    for n in PARAMS:
        p = getattr(model, n)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p is not old[n] and p.is_contiguous()
        assert torch.equal(p.detach(), before[n][keep]), n
        st = model.optimizer.state[p]
        assert old[n] not in model.optimizer.state
        assert torch.equal(st["exp_avg"], moments[n]["exp_avg"][keep]) and torch.equal(st["exp_avg_sq"], moments[n]["exp_avg_sq"][keep]), n
        assert float(st["step"]) == 2.0
        assert sum(any(q is p for q in gr["params"]) for gr in model.optimizer.param_groups) == 1
    assert torch.equal(model.aggregated_mask, mask) and int(torch.count_nonzero(model.aggregated_mask)) == Pn
    assert torch.equal(model._mask_index, index) and model._mask_index.dtype == torch.int64
    assert model._conf_static is conf_before, "conf_static is per pixel: it stays"
    assert [gr["name"] for gr in model.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "conf_static"]
    # the optimizer goes on, and its state loads into a fresh one
    for n in PARAMS + ("_conf_static",):
        getattr(model, n).grad = torch.randn(getattr(model, n).shape, generator=g)
    model.optimizer.step()
    assert float(model.optimizer.state[model._xyz]["step"]) == 3.0 and torch.isfinite(model._xyz).all()
    fresh = copy.deepcopy(model)
    fresh.training_setup(opt)
    fresh.optimizer.load_state_dict(model.optimizer.state_dict())
    assert torch.equal(fresh.optimizer.state[fresh._opacity]["exp_avg"], model.optimizer.state[model._opacity]["exp_avg"])
    assert model.optimizer_cam.state_dict()["param_groups"] == cam_state["param_groups"]


def test_nan_is_kept_negative_conf_is_dropped_and_the_guards_hold():
    from das3r_amd.prune import keep_mask, prune_points
    raw = torch.tensor([[2.0], [2.0], [float("nan")], [2.0], [-9.0]])
    conf = torch.tensor([1.0, -0.5, 1.0, float("nan"), 1.0])
    assert keep_mask(raw, conf, None, 0.005).tolist() == [True, False, True, True, False]
    assert keep_mask(raw, conf, torch.tensor([4, 3, 2, 1, 0]), 0.005).tolist() == [True, True, True, False, False]
    sc = torch.log(torch.tensor([[0.1, 0.1, 0.3], [0.1, 0.1, 0.1], [0.1, float("nan"), 0.5], [0.2, 0.2, 0.2], [0.1, 0.1, 0.1]]))
    assert keep_mask(raw, torch.ones(5), None, 0.0, sc, 0.25).tolist() == [False, True, True, True, True]
    assert keep_mask(raw, torch.ones(5), None, 0.0, sc, 0.0).all() and keep_mask(raw, torch.ones(5), None, 0.0, sc, -1.0).all()
    # an event that would keep nothing is skipped with a warning; nothing to drop changes nothing
    model = _host_model(seed=4)
    xyz, mask = model._xyz, model.aggregated_mask
    with pytest.warns(UserWarning, match="would drop all"):
        info = prune_points(model, min_opacity=2.0)
    assert info["after"] == info["before"] and model._xyz is xyz and model.aggregated_mask is mask
    info = prune_points(model, min_opacity=-1.0)
    assert info["dropped"] == 0 and model._xyz is xyz and model.aggregated_mask is mask


def test_a_loaded_model_compacts_its_per_gaussian_confidence():
    """offline.load_trained_model's model: plain tensors, no aggregated_mask, conf_static [P, 1] — the identity case of the index."""
    from das3r_amd.model import SplatModel
    from das3r_amd.prune import prune_points
    g = torch.Generator().manual_seed(8)
    m = SplatModel(1)
    P = 300
    m._xyz, m._features_dc, m._features_rest = torch.randn(P, 3, generator=g), torch.randn(P, 1, 3, generator=g), torch.randn(P, 3, 3, generator=g)
    m._scaling, m._rotation = torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g)
    m._opacity, m._conf_static = torch.randn(P, 1, generator=g) * 3, torch.rand(P, 1, generator=g)
    m.__dict__["_das3r_eval"] = object()
    keep = ~((torch.sigmoid(m._opacity) * m._conf_static).reshape(-1) < torch.tensor(1 / 255, dtype=torch.float32))
    before = {n: getattr(m, n).clone() for n in PARAMS + ("_conf_static",)}
    info = prune_points(m, min_opacity=1 / 255)
    assert info["after"] == int(keep.sum()) < P
    for n in PARAMS + ("_conf_static",):
        assert torch.equal(getattr(m, n), before[n][keep]) and not isinstance(getattr(m, n), torch.nn.Parameter), n
    assert "_das3r_eval" not in m.__dict__ and not hasattr(m, "aggregated_mask")


@pytest.mark.parametrize("degree", [0, 1])
def test_fused_adam_state_surgery_keeps_compact_sh_moments_compact(degree):
    """FusedAdam's state on host tensors (its step needs a device; its state does not): moments keyed by parameter, the SH moments in
    their compact [P, cols, 3] shape (cols = 0 at degree 0), integer step counts."""
    from das3r_amd.fused import FusedAdam
    from das3r_amd.prune import prune_points
    model = _host_model(seed=degree + 1)
    P = model._xyz.shape[0]
    groups = [{"params": [getattr(model, n)], "lr": 1e-3, "name": n, **({"sh_rest": True} if n == "_features_rest" else {})} for n in PARAMS]
    model.optimizer = FusedAdam(groups + [{"params": [model._conf_static], "lr": 3e-3, "name": "conf_static"}], lr=0.0, eps=1e-15)
    model.optimizer.set_active_sh_degree(degree)
    model.active_sh_degree = degree
    g = torch.Generator().manual_seed(2)
    cols = (degree + 1) ** 2 - 1
    for n in PARAMS:
        p = getattr(model, n)
        shape = (P, cols, 3) if n == "_features_rest" else tuple(p.shape)
        model.optimizer.state[p] = dict(step=7, exp_avg=torch.randn(*shape, generator=g), exp_avg_sq=torch.rand(*shape, generator=g))
    conf_state = model.optimizer.state[model._conf_static] = dict(step=7, exp_avg=torch.zeros_like(model._conf_static), exp_avg_sq=torch.zeros_like(model._conf_static))
    model._fast_state = object()
    keep, mask, index = _restatement(model, 0.005)
    old = {n: getattr(model, n) for n in PARAMS}
    moments = {n: dict(model.optimizer.state[old[n]]) for n in PARAMS}
    prune_points(model, min_opacity=0.005)
    Pn = int(keep.sum())
    for n in PARAMS:
        p = getattr(model, n)
        st = model.optimizer.state[p]
        assert old[n] not in model.optimizer.state and st["step"] == 7 and isinstance(st["step"], int)
        assert torch.equal(st["exp_avg"], moments[n]["exp_avg"][keep]) and torch.equal(st["exp_avg_sq"], moments[n]["exp_avg_sq"][keep])
        assert any(q is p for gr in model.optimizer.param_groups for q in gr["params"])
    assert tuple(model.optimizer.state[model._features_rest]["exp_avg"].shape) == (Pn, cols, 3)
    assert model.optimizer.state[model._conf_static] is conf_state and model.optimizer.handles_compact_sh(model._features_rest)
    assert "_fast_state" not in model.__dict__
    assert torch.equal(model.aggregated_mask, mask) and torch.equal(model._mask_index, index)
    sd = model.optimizer.state_dict()   # full-shaped moments leave, as torch.optim.Adam holds them
    assert tuple(sd["state"][2]["exp_avg"].shape) == (Pn, 15, 3)
    model.oneupSHdegree()               # the compact moments grow with zeros at the pruned size
    st = model.optimizer._sh_state(model._features_rest)
    assert tuple(st["exp_avg"].shape) == (Pn, (degree + 2) ** 2 - 1, 3) and torch.equal(st["exp_avg"][:, :cols], moments["_features_rest"]["exp_avg"][keep])


def test_the_schedule_is_off_by_default_and_in_the_loop_state():
    from das3r_amd import farm
    from das3r_amd.model import OptimParams
    from das3r_amd.train import prune_due, prune_schedule
    o = OptimParams()
    assert (o.prune_from_iter, o.prune_interval, o.prune_until_iter, o.prune_min_opacity, o.prune_max_world_scale) == (0, 0, 0, 0.005, 0.0)
    assert prune_schedule(o) is None and not any(prune_due(prune_schedule(o), it) for it in range(0, 5000))
    args = farm.parser().parse_args([])
    kw = farm.prune_kwargs(args)
    assert kw == dict(prune_from=0, prune_interval=0, prune_until=0, prune_min_opacity=0.005, prune_max_world_scale=0.0)
    assert prune_schedule(OptimParams(prune_from_iter=kw["prune_from"], prune_interval=kw["prune_interval"], prune_until_iter=kw["prune_until"],
                                      prune_min_opacity=kw["prune_min_opacity"], prune_max_world_scale=kw["prune_max_world_scale"])) is None
    args = farm.parser().parse_args("--prune-from 100 --prune-interval 100 --prune-until 600 --prune-min-opacity 0.01".split())
    kw = farm.prune_kwargs(args)
    s = prune_schedule(OptimParams(prune_from_iter=kw["prune_from"], prune_interval=kw["prune_interval"], prune_until_iter=kw["prune_until"],
                                   prune_min_opacity=kw["prune_min_opacity"]))
    assert s == (100, 100, 600, 0.01, 0.0)
    assert [it for it in range(1, 1000) if prune_due(s, it)] == [100, 200, 300, 400, 500, 600]
    assert [it for it in range(1, 400) if prune_due((150, 100, 350, 0.005, 0.0), it)] == [200, 300]
    from das3r_amd import offline
    a = offline.parser().parse_args(["-m", "x", "-s", "y"])
    assert a.prune_min_opacity == 0.0 and a.write_pruned_ply is False


class _Stop(Exception):
    pass


def test_resume_with_other_prune_settings_is_refused(monkeypatch):
    """train() compares the checkpoint's schedule with the one it is given before it runs anything."""
    import random
    from das3r_amd import train as T
    from das3r_amd.model import OptimParams
    model = _host_model()
    model.training_setup(OptimParams())
    cams = [type("Cam", (), {"uid": u})() for u in range(3)]
    loop = dict(rng=random.Random(0).getstate(), stack=[0, 1], ema=torch.zeros(()), last_psnr=torch.zeros(()), library=None, depth_l1=(0.0, 0.0),
                prune=(100, 100, 600, 0.005, 0.0))

    def stop(*a, **k):
        raise _Stop()

    monkeypatch.setattr(T, "train_step", stop)
    same = OptimParams(prune_from_iter=100, prune_interval=100, prune_until_iter=600)
    with pytest.raises(_Stop):   # the same settings pass the check (and reach the first step)
        T.train(model, cams, same, 10, start_iteration=5, loop_state=dict(loop))
    for other in (OptimParams(prune_from_iter=100, prune_interval=100, prune_until_iter=600, prune_min_opacity=0.01), OptimParams(),
                  OptimParams(prune_from_iter=100, prune_interval=50, prune_until_iter=600)):
        with pytest.raises(T.ResumeMismatch, match="prun"):
            T.train(model, cams, other, 10, start_iteration=5, loop_state=dict(loop))
    old = dict(loop)
    del old["prune"]             # a checkpoint from before pruning: off
    with pytest.raises(_Stop):
        T.train(model, cams, OptimParams(), 10, start_iteration=5, loop_state=old)
    with pytest.raises(T.ResumeMismatch):
        T.train(model, cams, same, 10, start_iteration=5, loop_state=old)


def test_train_runs_the_events_the_schedule_names(monkeypatch):
    from das3r_amd import prune as PR
    from das3r_amd import train as T
    from das3r_amd.model import OptimParams
    model = _host_model()
    model.training_setup(OptimParams())
    cams = [type("Cam", (), {"uid": u})() for u in range(3)]
    events, steps = [], []
    monkeypatch.setattr(T, "train_step", lambda m, cam, opt, it, *a, **k: (steps.append(it), (torch.zeros(()), torch.zeros(()), None))[1])
    monkeypatch.setattr(PR, "prune_points", lambda m, **k: events.append((len(steps), k)))
    T.train(model, cams, OptimParams(prune_from_iter=4, prune_interval=2, prune_until_iter=9, prune_min_opacity=0.01, prune_max_world_scale=3.0), 12)
    assert steps == list(range(1, 13))
    assert events == [(it, dict(min_opacity=0.01, max_world_scale=3.0)) for it in (4, 6, 8)]
    events.clear()
    T.train(model, cams, OptimParams(), 12)
    assert events == []


def test_restore_to_another_size_drops_the_cached_pixel_index():
    from das3r_amd.model import OptimParams
    from das3r_amd.prune import mask_index, prune_points
    opt = OptimParams(iterations=100)
    small = _host_model(seed=6)
    small.training_setup(opt)
    prune_points(small, min_opacity=0.005)
    capture, extras = copy.deepcopy(small.capture()), copy.deepcopy(small.capture_extras())
    big = _host_model(seed=6)
    big.training_setup(opt)
    stale = mask_index(big)
    big._fast_state = object()
    assert stale.numel() > small._xyz.shape[0]
    big.restore(capture, opt, extras=extras)
    assert getattr(big, "_mask_index", None) is None and "_fast_state" not in big.__dict__
    assert torch.equal(mask_index(big), small._mask_index) and mask_index(big).numel() == big._xyz.shape[0]
    assert torch.equal(big.aggregated_mask, small.aggregated_mask)
