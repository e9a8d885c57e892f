"""GPU tests of voxel thinning (INTEGRATION.md "Voxel thinning"; das3r_amd/thin.py, csrc/thin.hip): the kernels against the torch form bit
for bit over sizes and layouts (one cell, own cells, random, lattices, boundaries and signs, non-finite coordinates and special scores), run to
run; the guards; the model surgery by the kernels against the torch path, and the three forms of the train step on a thinned model; the
initialisation rule; a thinned job reproducing and resuming itself; the offline renderer."""
import copy
import ctypes as C
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import util
from tests.test_thin_host import hand_made_cases

pytestmark = pytest.mark.gpu

PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
PARAMS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
SIZES = [1, 63, 64, 65, 257, 4096, 2 ** 17 + 3]
SHAPE = dict(frames=6, W=128, H=80, n_splats=6000)
NAN, INF = float("nan"), float("inf")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _special_scores(P, g):
    """Scores with ties, +-0, NaN and +-inf among them."""
    s = torch.randint(-3, 4, (P,), generator=g).float()
    u = torch.rand(P, generator=g)
    s[u < 0.08] = -0.0
    s[(u >= 0.08) & (u < 0.16)] = 0.0
    s[(u >= 0.16) & (u < 0.24)] = NAN
    s[(u >= 0.24) & (u < 0.28)] = INF
    s[(u >= 0.28) & (u < 0.32)] = -INF
    return s


def _layouts(P, seed):
    """(name, xyz [P, 3], scores or None, inv_edge) on the CPU."""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(P)
    out = []
    inside = 0.999 * torch.rand(P, 3, generator=g)
    out.append(("one-cell-distinct", inside, torch.randperm(P, generator=g).float(), 1.0))      # (a) maximal contention
    out.append(("one-cell-equal", inside, torch.full((P,), 0.25), 1.0))
    out.append(("one-cell-negative", inside - 7.0, _special_scores(P, g), 1.0))
    own = torch.stack([(i % 1024).float() - 512.0, (i // 1024).float() - 64.0, torch.zeros(P)], 1) + 0.5
    out.append(("own-cells", own, torch.rand(P, generator=g), 1.0))                               # (b)
    side = max((P / 4.0) ** (1.0 / 3.0), 1.0)
    rnd = (torch.rand(P, 3, generator=g) - 0.5) * side
    out.append(("random", rnd, torch.rand(P, generator=g), 1.0))                                  # (c) about 4 per cell
    out.append(("random-edge-0.3", rnd * 0.3, torch.rand(P, generator=g), float(torch.tensor(1 / 0.3, dtype=torch.float32))))
    k = ((i // 2) - P // 4).float()                                                               # (d) two points per cell, negative k included
    z = torch.zeros(P)
    for name, cols in (("lattice-x", (k, z, z)), ("lattice-y", (z, k, z)), ("lattice-z", (z, z, k))):
        out.append((name, torch.stack(cols, 1) + 0.5, torch.rand(P, generator=g), 1.0))
    kd = (((i // 2) % 2048) - 1024).float() * 1024.0                                              # (k 2^10, k 2^10, 0): -2^20 .. 2^20 - 2^10
    out.append(("lattice-diagonal", torch.stack([kd, kd, z], 1) + 0.5, torch.rand(P, generator=g), 1.0))
    bad = rnd.clone()                                                                             # (f) 3 % of the points not placeable
    u = torch.rand(P, generator=g)
    bad[u < 0.01, 0] = NAN
    bad[(u >= 0.01) & (u < 0.015), 1] = INF
    bad[(u >= 0.015) & (u < 0.02), 2] = -INF
    bad[(u >= 0.02) & (u < 0.025), 0] = float(2 ** 20)
    bad[(u >= 0.025) & (u < 0.03), 1] = -float(2 ** 20) - 1.0
    out.append(("special", bad, _special_scores(P, g), 1.0))
    return out


def _run_kernels(xyz, score, inv):
    from das3r_amd.thin import voxel_keep_kernels
    keep, count, info = voxel_keep_kernels(xyz, score, inv)
    torch.cuda.synchronize()
    return keep, count, info


def _check(name, xyz, score, inv, cpu_too):
    """The kernels twice (identical bytes) against the torch form on the device (and, for small inputs, on the host)."""
    from das3r_amd.thin import voxel_keep_torch
    xyz = xyz.cuda().contiguous()
    score = None if score is None else score.cuda().contiguous()
    keep, count, info = _run_kernels(xyz, score, inv)
    k2, c2, i2 = _run_kernels(xyz, score, inv)
    assert torch.equal(keep, k2) and torch.equal(count, c2) and torch.equal(info, i2), f"{name}: two runs differ"
    tk, tc = voxel_keep_torch(xyz, score, inv)
    assert keep.dtype == torch.uint8 and count.dtype == torch.int32 and bool((keep <= 1).all())
    bad = int((keep.view(torch.bool) != tk).sum())
    assert bad == 0, f"{name}: keep differs from the torch form at {bad} of {xyz.shape[0]} points"
    assert torch.equal(count, tc), f"{name}: count differs at {int((count != tc).sum())} points"
    assert info.tolist() == [int(tk.sum()), 0], (name, info.tolist(), int(tk.sum()))
    assert int(count.sum()) == xyz.shape[0]
    if cpu_too:
        hk, hc = voxel_keep_torch(xyz.cpu(), None if score is None else score.cpu(), inv)
        assert torch.equal(hk, tk.cpu()) and torch.equal(hc, tc.cpu()), f"{name}: the torch form differs between host and device"
    return int(tk.sum())


# ---------------------------------------------------------------------------------------------------------------- 1. kernels = torch form
@pytest.mark.parametrize("P", SIZES)
def test_kernels_equal_the_torch_form_exactly(P):
    kept = {}
    for name, xyz, score, inv in _layouts(P, 100 + P):
        kept[name] = _check(name, xyz, score, inv, cpu_too=P <= 4096)
        _check(name + " (no score)", xyz, None, inv, cpu_too=P <= 4096)
    assert kept["one-cell-distinct"] == kept["one-cell-equal"] == 1 and kept["own-cells"] == P
    assert kept["lattice-x"] == kept["lattice-y"] == kept["lattice-z"] == (P + 1) // 2
    if P >= 4096:
        assert 0.15 * P < kept["random"] < 0.5 * P and kept["special"] > kept["random"]


def test_kernels_equal_the_torch_form_on_the_boundary_and_sign_cases():
    for name, xyz, score, inv in hand_made_cases():
        x = torch.tensor(xyz, dtype=torch.float32)
        _check(name, x, torch.tensor(score, dtype=torch.float32), inv, cpu_too=True)
        _check(name + " (no score)", x, None, inv, cpu_too=True)


def test_kernels_equal_the_torch_form_at_a_million_points():
    P = 2 ** 20 + 3
    g = torch.Generator().manual_seed(8)
    xyz = (torch.rand(P, 3, generator=g) - 0.5) * (P / 4.0) ** (1.0 / 3.0)
    kept = _check("random 2^20 + 3", xyz, _special_scores(P, g), 1.0, cpu_too=False)
    assert 0.15 * P < kept < 0.5 * P
    _check("one cell 2^20 + 3", 0.999 * torch.rand(P, 3, generator=g), torch.rand(P, generator=g), 1.0, cpu_too=False)


def test_voxel_keep_takes_the_kernels_on_the_device():
    from das3r_amd.thin import inv_edge_of, voxel_keep, voxel_keep_torch
    g = torch.Generator().manual_seed(3)
    xyz, score = torch.rand(5000, 3, generator=g).cuda(), torch.rand(5000, generator=g).cuda()
    keep, count, kept = voxel_keep(xyz, score, edge=0.1, use_kernels=True)
    tk, tc = voxel_keep_torch(xyz, score, inv_edge_of(0.1))
    assert keep.dtype == torch.bool and torch.equal(keep, tk) and torch.equal(count, tc) and kept == int(tk.sum())
    k3, c3, n3 = voxel_keep(xyz, score, edge=0.1, use_kernels=False)
    assert torch.equal(k3, tk) and torch.equal(c3, tc) and n3 == kept
    with pytest.raises(RuntimeError, match="dense fp32"):
        voxel_keep(xyz.double(), score, edge=0.1, use_kernels=True)
    assert voxel_keep(xyz.t().contiguous().t(), score, edge=0.1)[2] == kept   # a view that is not dense: the torch form, the same answer


# ---------------------------------------------------------------------------------------------------------------- 2. guards
def test_guards():
    from das3r_amd import _lib
    lib = _lib.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    info = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    assert lib.das3r_thin_workspace_bytes(0) == 0
    assert lib.das3r_thin_voxels(0, None, None, C.c_float(1.0), None, None, _p(info), None, s) == 0
    torch.cuda.synchronize()
    assert info.tolist() == [0, 0]
    P = 1000
    xyz = torch.rand(P, 3, device="cuda")
    keep, count = torch.full((P,), 9, dtype=torch.uint8, device="cuda"), torch.full((P,), -5, dtype=torch.int32, device="cuda")
    n = int(lib.das3r_thin_workspace_bytes(P))
    assert n == 20 * 2048 + 4 * P
    assert int(lib.das3r_thin_workspace_bytes(2 ** 17 + 3)) == 20 * 2 ** 19 + 4 * (2 ** 17 + 3)
    guard = 4096
    buf = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    for bad in (0.0, -1.0, NAN, INF, -INF):
        info.fill_(77)
        assert lib.das3r_thin_voxels(P, _p(xyz), None, C.c_float(bad), _p(keep), _p(count), _p(info), _p(buf), s) == -1, bad
        assert "inv_edge" in _lib.last_error()
    for args in ((None, _p(keep), _p(count), _p(info), _p(buf)), (_p(xyz), None, _p(count), _p(info), _p(buf)), (_p(xyz), _p(keep), None, _p(info), _p(buf)),
                 (_p(xyz), _p(keep), _p(count), None, _p(buf)), (_p(xyz), _p(keep), _p(count), _p(info), None)):
        assert lib.das3r_thin_voxels(P, args[0], None, C.c_float(1.0), args[1], args[2], args[3], args[4], s) == -1
        assert "das3r_thin_voxels" in _lib.last_error()
    assert lib.das3r_thin_voxels(-1, _p(xyz), None, C.c_float(1.0), _p(keep), _p(count), _p(info), _p(buf), s) == -1
    torch.cuda.synchronize()
    assert info.tolist() == [77, 77] and bool((keep == 9).all()) and bool((count == -5).all()) and bool((buf == 0xA5).all()), "a refused call wrote something"
    # a workspace of exactly the stated size: the guard region behind it comes back untouched
    assert lib.das3r_thin_voxels(P, _p(xyz), None, C.c_float(8.0), _p(keep), _p(count), _p(info), _p(buf), s) == 0
    torch.cuda.synchronize()
    assert bool((buf[n:] == 0xA5).all()), "the kernels wrote behind das3r_thin_workspace_bytes(P)"
    from das3r_amd.thin import voxel_keep_torch
    tk, tc = voxel_keep_torch(xyz, None, 8.0)
    assert torch.equal(keep.view(torch.bool), tk) and torch.equal(count, tc) and info.tolist() == [int(tk.sum()), 0]


# ---------------------------------------------------------------------------------------------------------------- 3. model surgery
_SEQ = {}


def _sequence():
    """consistent_sequence at SHAPE, computed once and left unchanged."""
    if "seq" not in _SEQ:
        from das3r_amd.train import consistent_sequence
        _SEQ["seq"] = consistent_sequence(seed=0, moving=True, **SHAPE)
    return _SEQ["seq"]


def _footprint(heldout):
    from das3r_amd.train import sequence_footprint
    return sequence_footprint(_sequence(), heldout=heldout)


def _moments(model):
    out = {}
    for n in PARAMS + ("_conf_static",):
        st = model.optimizer.state.get(getattr(model, n))
        if st is not None:
            out[n] = (float(st["step"]), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return out


@pytest.mark.parametrize("fused", [True, False], ids=["fused-adam", "torch-adam"])
def test_thin_model_by_the_kernels_equals_the_torch_path_bitwise(fused):
    """A few steps (Adam moments of the optimizer kind), then the same state thinned twice: parameters, both moments, aggregated_mask and
    _mask_index are torch.equal."""
    from das3r_amd.model import OptimParams
    from das3r_amd.thin import thin_model
    from das3r_amd.train import build_from_sequence, train_step
    model, cams = build_from_sequence(_sequence())
    opt = OptimParams(iterations=100)
    model.training_setup(opt, fused=fused)
    bg = torch.zeros(3, device="cuda")
    for it, u in enumerate([0, 3, 1], start=1):
        train_step(model, cams[u], opt, it, PIPE, bg, fused=fused)
    model.__dict__.pop("_fast_state", None)
    P = model._xyz.shape[0]
    a, b = copy.deepcopy(model), copy.deepcopy(model)
    edge = 1.0 * _footprint(False)
    ia, ib = thin_model(a, edge), thin_model(b, edge, use_kernels=False)
    print(f"[thin_model {'fused' if fused else 'torch'} adam] P {P} -> {ia['after']} at edge {edge:.5g}")
    assert ia["path"] == "kernels" and ib["path"] == "torch" and ia["edge"] == ib["edge"] == edge
    assert ia["after"] == ib["after"] and 0 < ia["after"] < P, (ia, ib)
    for n in PARAMS:
        assert torch.equal(getattr(a, n).detach(), getattr(b, n).detach()), n
        assert getattr(a, n).shape[0] == ia["after"]
    ma, mb = _moments(a), _moments(b)
    assert set(ma) == set(mb) == set(_moments(model)) and len(ma) >= 5
    for n in ma:
        assert ma[n][0] == mb[n][0] and torch.equal(ma[n][1], mb[n][1]) and torch.equal(ma[n][2], mb[n][2]), n
    assert torch.equal(a.aggregated_mask, b.aggregated_mask) and int(torch.count_nonzero(a.aggregated_mask)) == ia["after"]
    assert torch.equal(a._mask_index, b._mask_index) and torch.equal(a._mask_index, torch.nonzero(a.aggregated_mask.reshape(-1)).reshape(-1))
    assert torch.equal(a._opacity.detach(), model._opacity.detach()[a_keep(model, edge)])   # opacities untouched: the survivors' own rows


def a_keep(model, edge):
    from das3r_amd.thin import default_score, voxel_keep
    keep, _, _ = voxel_keep(model._xyz.detach(), default_score(model), edge=edge, use_kernels=False)
    return keep & ~(default_score(model) < 0)


FORMS = {"torch-glue": dict(fused=False), "fused-autograd": dict(fused=True, fast_step=False), "fast-step": dict(fused=True, fast_step=True)}


def test_the_three_forms_of_the_train_step_agree_on_a_thinned_model():
    """The same thinned model stepped once by the torch glue, the fused autograd form and the direct form, each from a fresh optimizer: the
    losses agree within GRAD_REL_TOL and the first Adam moments — (1 - beta1) x the step's gradients — under assert_grad_close."""
    from das3r_amd import fast_step
    from das3r_amd.model import OptimParams
    from das3r_amd.thin import thin_model
    from das3r_amd.train import build_from_sequence, train_step
    edge = 1.0 * _footprint(False)
    bg = torch.zeros(3, device="cuda")
    out = {}
    for form, how in FORMS.items():
        model, cams = build_from_sequence(_sequence())
        opt = OptimParams(iterations=100)
        model.training_setup(opt, fused=how["fused"])
        info = thin_model(model, edge)
        assert info["path"] == "kernels" and info["dropped"] > 0
        if "fast_step" in how:
            model.fast_step = how["fast_step"]
        assert (how["fused"] and fast_step.available(model, PIPE)) == (form == "fast-step")
        loss = float(train_step(model, cams[2], opt, 1, PIPE, bg, fused=how["fused"])[0])
        torch.cuda.synchronize()
        out[form] = (loss, info["after"], {n: model.optimizer.state[getattr(model, n)]["exp_avg"].detach().cpu().numpy()
                                          for n in ("_xyz", "_features_dc", "_opacity", "_scaling", "_rotation")})
    ref = out["torch-glue"]
    for form in ("fused-autograd", "fast-step"):
        loss, after, m = out[form]
        print(f"[{form}] P {after}; loss {loss:.9g} vs torch glue {ref[0]:.9g} (rel {abs(loss - ref[0]) / abs(ref[0]):.3g})")
        assert after == ref[1]
        for n in m:
            d = float(np.abs(m[n] - ref[2][n]).max()) / max(float(np.abs(ref[2][n]).max()), 1e-30)
            print(f"[{form}] {n}: first moment max |delta| / max |ref| = {d:.3g} (bar {util.GRAD_REL_TOL})")
        assert abs(loss - ref[0]) <= util.GRAD_REL_TOL * abs(ref[0])
        for n in m:
            util.assert_grad_close(m[n], ref[2][n], f"{form} {n} first moment on a thinned model")


# ---------------------------------------------------------------------------------------------------------------- 4. initialisation
@pytest.mark.parametrize("mode", ["coverage", "reference"])
def test_initialisation_follows_the_rule(mode):
    from das3r_amd import thin
    from das3r_amd.knn import distCUDA2
    from das3r_amd.losses import inverse_sigmoid
    from das3r_amd.model import depth_to_points
    from das3r_amd.train import build_from_sequence, split_sequence
    seq = _sequence()
    model, cams, _test = build_from_sequence(seq, heldout=True, thin_relative=1.0, thin_opacity=mode)
    plain, _, _ = build_from_sequence(seq, heldout=True)
    assert plain.thin_info is None and model.thin_init == ("relative", 1.0, mode)
    tr, _ = split_sequence(seq)
    sel = torch.tensor(tr, device="cuda")
    F = len(tr)
    edge = 1.0 * _footprint(True)
    assert model.thin_info["edge"] == edge and model.thin_info["before"] == plain._xyz.shape[0]
    pts = depth_to_points(seq["K"][sel].float(), seq["cam2world"][sel].float(), seq["depths"][sel].float()).reshape(-1, 3)
    mask0 = seq["confs"][sel].reshape(-1) > 0
    pts = pts[mask0].contiguous()
    assert torch.equal(pts, plain._xyz.detach())
    # P = the distinct placeable cells + the points that are not placeable (an independent count: unique ROWS of cells)
    prod = pts * torch.tensor(thin.inv_edge_of(edge), dtype=torch.float32, device="cuda")
    cell = torch.floor(prod)
    placeable = (torch.isfinite(prod) & (cell >= -2.0 ** 20) & (cell < 2.0 ** 20)).all(dim=1)
    cells = int(torch.unique(cell[placeable].to(torch.int64), dim=0).shape[0])
    P = model._xyz.shape[0]
    print(f"[init {mode}] P {pts.shape[0]} -> {P} ({cells} cells, {int((~placeable).sum())} not placeable) at edge {edge:.5g}, F = {F}")
    assert P == cells + int((~placeable).sum()) == model.thin_info["after"] and P < pts.shape[0]
    keep, count = thin.voxel_keep_torch(pts, seq["confs"][sel].reshape(-1)[mask0].float(), thin.inv_edge_of(edge))
    pixels = torch.nonzero(mask0).reshape(-1)
    want = torch.zeros_like(mask0)
    want[pixels[keep]] = True
    assert torch.equal(model.aggregated_mask, want), "the cleared mask bits are exactly the losers"
    assert torch.equal(model._xyz.detach(), pts[keep])
    scales = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(pts[keep].contiguous()), 0.0000001)))[..., None].repeat(1, 3)
    assert torch.equal(model._scaling.detach(), scales), "the scales are distCUDA2 of the survivors"
    base = (1.0 / F) * torch.ones(P, 1, device="cuda")
    opac = base if mode == "reference" else thin.coverage_opacity(count[keep], base, F)
    assert torch.equal(model._opacity.detach(), inverse_sigmoid(opac))
    c = count[keep]
    if mode == "coverage":
        assert bool((c > 1).any())
        one = (c == 1).reshape(-1)
        assert torch.equal(model._opacity.detach()[one], inverse_sigmoid(base)[one])
        assert float(torch.sigmoid(model._opacity.detach()).max()) <= 0.99 + 1e-6
        assert bool((torch.sigmoid(model._opacity.detach()[~one]) > 1.0 / F).all())
    assert int(c.sum()) == pts.shape[0]


def _manual_job(iterations, **thin_kw):
    """A fused job by hand (the loss of every iteration is kept): -> (model, [iterations] losses)."""
    from das3r_amd import _lib
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, train_step
    _lib.forget_shapes()
    model, cams, _test = build_from_sequence(_sequence(), heldout=True, **thin_kw)
    opt = OptimParams(iterations=iterations)
    model.training_setup(opt, fused=True)
    bg = torch.zeros(3, device="cuda")
    losses = [train_step(model, cams[(7 * it) % len(cams)], opt, it, PIPE, bg, fused=True)[0].clone() for it in range(1, iterations + 1)]
    torch.cuda.synchronize()
    return model, torch.stack(losses)


def test_an_edge_below_the_point_spacing_leaves_a_job_bit_identical():
    from das3r_amd.thin import voxel_keep
    plain, trace = _manual_job(50)
    from das3r_amd.train import build_from_sequence
    fresh, _, _ = build_from_sequence(_sequence(), heldout=True)
    P = fresh._xyz.shape[0]
    edge = 3e-4 * _footprint(True)
    for _ in range(6):   # an edge at which no two points share a cell
        if voxel_keep(fresh._xyz.detach(), None, edge=edge)[2] == P:
            break
        edge *= 0.5
    assert voxel_keep(fresh._xyz.detach(), None, edge=edge)[2] == P
    thinned, trace_t = _manual_job(50, thin_edge=edge)
    assert thinned.thin_info["before"] == thinned.thin_info["after"] == P
    assert torch.equal(trace, trace_t), "the loss trace"
    for n in PARAMS + ("_conf_static", "Q", "T"):
        assert torch.equal(getattr(plain, n).detach(), getattr(thinned, n).detach()), n
    assert torch.equal(plain.aggregated_mask, thinned.aggregated_mask)


# ---------------------------------------------------------------------------------------------------------------- 5. a thinned job
def test_a_thinned_job_finishes_reproduces_itself_and_resumes_bit_identical(tmp_path):
    """200 fused iterations from thin_relative = 1.0 with the held-out split, a checkpoint at iteration 100: a second run ends bit-identical,
    the job resumed from the checkpoint too; the setting is in the checkpoint's loop state, and a resume with another one is refused."""
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.train import ResumeMismatch, latest_checkpoint
    dev = torch.device("cuda:0")
    seq = _sequence()
    full_dir, res_dir, bad_dir = str(tmp_path / "full"), str(tmp_path / "resumed"), str(tmp_path / "other")
    k1, k2, k3 = {}, {}, {}
    kw = dict(fused=True, seq=seq, thin_init_relative=1.0)
    full = run_sequence_job(0, 200, dev, out_dir=full_dir, keep=k1, checkpoint_every=100, **kw)
    P0 = (SHAPE["frames"] - 1) * SHAPE["W"] * SHAPE["H"]
    print(f"[thinned job] P {P0} -> {full['n_splats']}; held-out static PSNR {full['psnr']:.4f} dB")
    assert full["ok"] == 1 and np.isfinite(full["psnr"]) and 0 < full["n_splats"] < P0
    assert latest_checkpoint(full_dir)[1] == 100
    extras = torch.load(os.path.join(full_dir, "chkpnt100.das3r.pth"), weights_only=False)
    assert extras["loop"]["thin"] == (("relative", 1.0, "coverage"), 0.0)
    again = run_sequence_job(0, 200, dev, keep=k2, **kw)
    for d in (res_dir, bad_dir):
        os.makedirs(d)
        for f in ("chkpnt100.pth", "chkpnt100.das3r.pth"):
            shutil.copy(os.path.join(full_dir, f), os.path.join(d, f))
    res = run_sequence_job(0, 200, dev, out_dir=res_dir, resume=True, keep=k3, checkpoint_every=100, **kw)
    a = k1[0][0]
    for what, rec, other in (("a second run", again, k2[0][0]), ("the resumed job", res, k3[0][0])):
        assert rec["ok"] == 1 and rec["n_splats"] == full["n_splats"] and rec["psnr"] == full["psnr"], what
        for n in PARAMS + ("_conf_static", "Q", "T"):
            assert torch.equal(getattr(a, n).detach(), getattr(other, n).detach()), f"{n}: {what} must end bit-identical"
        assert torch.equal(a.aggregated_mask, other.aggregated_mask)
    for other in (dict(thin_init_relative=2.0), dict(thin_init_relative=1.0, thin_opacity="reference"), {}):
        with pytest.raises(ResumeMismatch, match="thin"):
            run_sequence_job(0, 200, dev, out_dir=bad_dir, resume=True, fused=True, seq=seq, checkpoint_every=100, **other)


def test_prune_events_thin_too():
    """--prune-thin-relative: the events of a pruning schedule also drop the voxel losers; the job finishes smaller than it began."""
    from das3r_amd.farm import run_sequence_job
    keep = {}
    rec = run_sequence_job(0, 60, torch.device("cuda:0"), fused=True, seq=_sequence(), keep=keep, prune_from=20, prune_interval=20, prune_until=40,
                           prune_thin_relative=1.0)
    P0 = (SHAPE["frames"] - 1) * SHAPE["W"] * SHAPE["H"]
    model = keep[0][0]
    assert rec["ok"] == 1 and np.isfinite(rec["psnr"]) and rec["n_splats"] == model._xyz.shape[0] < P0
    assert int(torch.count_nonzero(model.aggregated_mask)) == rec["n_splats"]


# ---------------------------------------------------------------------------------------------------------------- 6. offline
def test_offline_thins_renders_and_writes_a_ply_that_reloads(tmp_path):
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.io_formats import load_gaussians_ply
    from das3r_amd.offline import load_trained_model, render_sets
    from das3r_amd.thin import thin_model
    seq = _sequence()
    out = str(tmp_path / "job")
    rec = run_sequence_job(0, 60, torch.device("cuda:0"), fused=True, seq=seq, out_dir=out)
    assert rec["ok"] == 1
    edge = 1.0 * _footprint(False)
    it, imgs = render_sets(out, seq, fused=True, thin_edge=edge, write_pruned_ply=True)
    renders = os.path.join(out, "interp", "ours_60", "renders")
    assert it == 60 and len(imgs) == SHAPE["frames"] and sorted(os.listdir(renders)) == [f"{k:05d}.png" for k in range(SHAPE["frames"])]
    assert all(bool(torch.isfinite(i).all()) for i in imgs)
    model, _ = load_trained_model(out, 60)
    P = model._xyz.shape[0]
    info = thin_model(model, edge)
    assert info["path"] == "kernels" and 0 < info["after"] < P
    g = load_gaussians_ply(os.path.join(out, "point_cloud", "iteration_60", "point_cloud_pruned.ply"))
    for name, attr in (("xyz", "_xyz"), ("features_dc", "_features_dc"), ("features_rest", "_features_rest"), ("opacity", "_opacity"),
                       ("conf_static", "_conf_static"), ("scaling", "_scaling"), ("rotation", "_rotation")):
        assert np.array_equal(g[name], getattr(model, attr).detach().cpu().numpy()), name
    # --thin-relative takes the footprint from the sequence's depth maps and intrinsics
    it2, imgs2 = render_sets(out, seq, write=False, fused=True, thin_relative=1.0)
    assert it2 == 60 and len(imgs2) == len(imgs)
    for k, (x, y) in enumerate(zip(imgs2, imgs)):
        util.assert_color_close(x.cpu().numpy(), y.cpu().numpy(), f"offline view {k}: thin_relative 1.0 vs the same edge in world units")
