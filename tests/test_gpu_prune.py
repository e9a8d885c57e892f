"""GPU tests of pruning (INTEGRATION.md "Pruning"; das3r_amd/prune.py, csrc/prune.hip): the selection against its formula, the compaction
against t[keep] bit for bit, the model surgery by the kernels against the torch form, "pruning at 1/255 changes nothing that is left" in
the three forms of the train step, the exact count at initialisation, a pruned job against the unpruned baselines of the parent commit,
resume, and the offline renderer."""
import copy
import ctypes as C
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

PIPE = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
PARAMS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
SIZES = [1, 63, 64, 65, 1000, 2 ** 20 + 3]
SMALL = dict(frames=12, W=256, H=104, focal=300.0, n_splats=8000)   # tests/test_gpu_depth_train.py's SMALL
# docs/ledger.md (cc): held-out static-region PSNR of the UNPRUNED job (consistent_sequence(seed, **SMALL), held-out split, fused, 600
# iterations, job seed = sequence seed) run at the parent commit (8c8196e), and the margin = max(max - min of the three, 0.3 dB: SURVEY C11)
BASELINE_PSNR = {0: 42.74244689941406, 1: 44.507171630859375, 2: 44.761226654052734}   # (each reproduced bit for bit by a second run)
PSNR_MARGIN = max(max(BASELINE_PSNR.values()) - min(BASELINE_PSNR.values()), 0.3)   # 2.019 dB: the spread of the three seeds


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _library_eff_and_scales(raw, conf, index, scaling):
    """The opacity and the scales das3r_pretransform_forward hands the rasterizer for these inputs (identity pose): pre_opacity / pre_scale,
    the helpers the selection must use."""
    from das3r_amd import _lib
    lib = _lib.load()
    P = raw.shape[0]
    dev = raw.device
    mats = torch.zeros(28, device=dev)
    xyz, rot = torch.zeros(P, 3, device=dev), torch.zeros(P, 4, device=dev)
    sc = scaling if scaling is not None else torch.zeros(P, 3, device=dev)
    means, rots, scales, opac = torch.empty(P, 3, device=dev), torch.empty(P, 4, device=dev), torch.empty(P, 3, device=dev), torch.empty(P, 1, device=dev)
    rc = lib.das3r_pretransform_forward(P, _p(xyz), _p(rot), _p(sc), _p(raw), _p(conf), _p(index), _p(mats), C.c_void_p(mats.data_ptr() + 36),
                                        C.c_void_p(mats.data_ptr() + 48), _p(means), _p(rots), _p(scales), _p(opac), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "das3r_pretransform_forward")
    return opac.reshape(-1), scales


def _select_inputs(P, seed, identity):
    g = torch.Generator().manual_seed(seed)
    raw = (4.0 * torch.randn(P, 1, generator=g) - 3.0)
    n_conf = P if identity else 2 * P + 7
    conf = torch.rand(n_conf, generator=g)
    conf[torch.rand(n_conf, generator=g) < 0.15] = 0.0
    conf[torch.rand(n_conf, generator=g) < 0.05] = -0.3          # the parameter is unclamped
    conf[torch.rand(n_conf, generator=g) < 0.05] = float("nan")
    raw[torch.rand(P, generator=g) < 0.03] = float("nan")
    index = None if identity else torch.sort(torch.randperm(n_conf, generator=g)[:P]).values
    scaling = -2.0 + 0.5 * torch.randn(P, 3, generator=g)
    scaling[torch.rand(P, generator=g) < 0.02, 1] = float("nan")
    also = torch.rand(P, generator=g) < 0.1
    return raw, conf, index, scaling, also


# ---------------------------------------------------------------------------------------------------------------- 1. select = formula
@pytest.mark.parametrize("identity", [True, False])
@pytest.mark.parametrize("P", SIZES)
def test_select_equals_the_formula_exactly(P, identity):
    """Keep mask, new rows and count of das3r_prune_select against `~(eff < t) [& ~(max exp(s) > limit)] [& ~also]` evaluated by torch on
    the opacities and scales the library's own pre-transform writes for the same inputs (pre_opacity / pre_scale: the same fp32
    expression, the same bits), with each optional criterion on and off, NaN and negative confidences among the inputs.  Against
    prune.keep_mask (torch.sigmoid / torch.exp, whose last bit may differ from the library's) the decisions must agree on every row whose
    opacity is not within 8 ulp of the threshold (and whose largest scale is not within 8 ulp of the limit): exp to 2 ulp and one rounding
    each for the add, the divide and the multiply, on either side."""
    from das3r_amd.prune import keep_mask, select
    raw, conf, index, scaling, also = (None if t is None else t.cuda().contiguous() for t in _select_inputs(P, 11 + P, identity))
    eff, scales = _library_eff_and_scales(raw, conf, index, scaling)
    t = 0.005
    t32 = torch.tensor(t, dtype=torch.float32, device="cuda")
    nanmax = torch.where(torch.isnan(scales).any(dim=1), torch.full((P,), float("nan"), device="cuda"), scales.max(dim=1).values)
    seen_drop = seen_nan_kept = 0
    for limit, use_also in ((0.0, False), (0.25, False), (0.0, True), (0.25, True), (-1.0, False)):
        drop = eff < t32
        if limit > 0:
            drop = drop | (nanmax > torch.tensor(limit, dtype=torch.float32, device="cuda"))
        if use_also:
            drop = drop | also
        keep = ~drop
        dst, count = select(raw, conf, index, t, scaling if limit != 0.0 else None, limit, also if use_also else None)
        torch.cuda.synchronize()
        got_keep = dst >= 0
        assert torch.equal(got_keep, keep), (P, identity, limit, use_also, int((got_keep != keep).sum()))
        assert int(count[0]) == int(keep.sum())
        expect_rows = (torch.cumsum(keep.to(torch.int32), 0) - 1).to(torch.int32)
        assert torch.equal(dst[keep], expect_rows[keep]) and bool((dst[~keep] == -1).all()), "new rows = exclusive prefix sum of the keep flags"
        seen_drop += int(drop.sum())
        seen_nan_kept += int((torch.isnan(eff) & keep).sum())
        # the torch form of the decision (the oracle of the model-level tests) away from the threshold
        tk = keep_mask(raw, conf, index, t, scaling if limit != 0.0 else None, limit, also if use_also else None)
        near = (eff - t32).abs() <= 8 * 2.0 ** -23 * t
        if limit > 0:
            near = near | ((nanmax - limit).abs() <= 8 * 2.0 ** -23 * limit)
        assert torch.equal(tk[~near], keep[~near])
    if P >= 1000:
        assert seen_drop > 0 and seen_nan_kept > 0
    # negative confidence counts as below the threshold; scaling given with a limit <= 0 is the criterion switched off
    neg = (conf if index is None else conf[index]) < 0
    dst, _ = select(raw, conf, index, t, scaling, 0.0, None)
    assert bool((dst[neg & ~torch.isnan(raw.reshape(-1))] == -1).all())
    assert torch.equal(dst >= 0, ~(eff < t32))


def test_select_of_nothing_and_guards():
    from das3r_amd.prune import compact, select
    e = torch.empty(0, 1, device="cuda")
    dst, count = select(e, torch.empty(0, device="cuda"), None, 0.005)
    torch.cuda.synchronize()
    assert dst.numel() == 0 and int(count[0]) == 0
    assert compact(dst, 0, [torch.empty(0, 3, device="cuda")])[0].shape == (0, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        select(torch.zeros(4, 1), torch.zeros(4), None, 0.005)


# ---------------------------------------------------------------------------------------------------------------- 2. compact = t[keep]
ROW_BYTES = (4, 8, 12, 16, 36, 108, 180, 192)


def _keep_of(P, fraction, seed):
    g = torch.Generator().manual_seed(seed)
    if fraction == "none":
        return torch.zeros(P, dtype=torch.bool)
    if fraction == "all":
        return torch.ones(P, dtype=torch.bool)
    return torch.rand(P, generator=g) < fraction


@pytest.mark.parametrize("fraction", ["none", "all", 0.001, 0.5, 0.97])
@pytest.mark.parametrize("P", SIZES)
def test_compact_equals_boolean_indexing_bit_for_bit(P, fraction):
    """Sixteen tensors in one call — fp32 rows of 4, 8, 12, 16, 36, 108, 180 and 192 bytes (twice: one set at 16-byte aligned addresses, one
    set offset by 4 bytes), the int64 index among the 8-byte ones — against t[keep]; a seventeenth and a zero-width tensor ([P, 0, 3]: compact
    SH moments at degree 0) go through the host layer's chunking.  The new rows are the selection's own (also_drop carries the keep mask)."""
    from das3r_amd.prune import compact, select
    keep = _keep_of(P, fraction, 5 + P).cuda()
    dst, count = select(torch.zeros(P, 1, device="cuda"), torch.ones(P, device="cuda"), None, 0.005, None, 0.0, ~keep)
    kept = int(count[0])
    assert kept == int(keep.sum())
    g = torch.Generator().manual_seed(P)
    tensors = []
    for rb in ROW_BYTES:
        n = rb // 4
        a = torch.randn(P, n, generator=g).cuda()
        backing = torch.empty(P * n + 1, device="cuda")      # the same rows at an address that is 4 bytes off a 16-byte boundary
        b = backing[1:].view(P, n)
        b.copy_(torch.randn(P, n, generator=g))
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4 and b.is_contiguous()
        tensors += [a, b]
    tensors[2] = torch.randint(-2 ** 62, 2 ** 62, (P,), generator=g, dtype=torch.int64).cuda()   # (8-byte rows: the pixel index)
    assert len(tensors) == 16
    tensors += [torch.randn(P, 15, 3, generator=g).cuda(), torch.empty(P, 0, 3, device="cuda")]
    out = compact(dst, kept, tensors)
    torch.cuda.synchronize()
    for t, o in zip(tensors, out):
        ref = t[keep]
        assert o.shape == ref.shape and o.dtype == t.dtype and o.is_contiguous()
        assert torch.equal(o.view(torch.uint8) if o.numel() else o, ref.contiguous().view(torch.uint8) if ref.numel() else ref), (P, fraction, tuple(t.shape))


def test_compact_refuses_what_it_cannot_do():
    from das3r_amd import _lib
    lib = _lib.load()
    dst = torch.arange(8, dtype=torch.int32, device="cuda")
    a, b = torch.zeros(8, 3, device="cuda"), torch.zeros(8, 3, device="cuda")
    arr = (_lib.PruneTensor * 1)()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    arr[0].src, arr[0].dst, arr[0].row_bytes = a.data_ptr(), a.data_ptr(), 12
    assert lib.das3r_prune_compact(8, 8, _p(dst), 1, arr, s) == -1 and "overlap" in _lib.last_error()
    arr[0].dst, arr[0].row_bytes = b.data_ptr(), 6
    assert lib.das3r_prune_compact(8, 8, _p(dst), 1, arr, s) == -1
    assert lib.das3r_prune_compact(8, 8, _p(dst), 17, arr, s) == -1


# ---------------------------------------------------------------------------------------------------------------- 3. model level
def _sequence_model(frames, W, H, seed, fused, torch_adam=False, iterations=100, drop=True):
    """A model from train.synthetic_sequence in a generic state (anisotropic, rotated: tests/test_gpu_trainstep.py `_pair` says why), of
    which — with `drop` — about 30 % of the Gaussians are rendered below 1/255: half through conf_static == 0, half through a low raw
    opacity.  Nobody sits near the threshold: the live ones are rendered at 1 / frames."""
    from das3r_amd.model import OptimParams
    from das3r_amd.train import build_from_sequence, synthetic_sequence
    seq = synthetic_sequence(frames=frames, W=W, H=H, focal=0.9 * W, n_splats=1500, seed=seed)
    model, cams = build_from_sequence(seq)
    gen = torch.Generator().manual_seed(7 + seed)
    with torch.no_grad():
        model._scaling += 0.4 * torch.randn(model._scaling.shape, generator=gen).cuda()
        model._rotation.copy_(torch.nn.functional.normalize(torch.randn(model._rotation.shape, generator=gen)).cuda())
        if drop:
            P = model._xyz.shape[0]
            u = torch.rand(P, generator=gen)
            model._opacity[(u < 0.15).cuda()] = -8.0                                  # sigmoid(-8) = 3.4e-4
            model._conf_static.view(-1)[((u >= 0.15) & (u < 0.30)).cuda()] = 0.0       # (every pixel is a Gaussian here: pixel = row)
    opt = OptimParams(iterations=iterations)
    model.training_setup(opt, fused=fused and not torch_adam)
    return model, cams, opt


def _moments(model):
    out = {}
    for n in PARAMS + ("_conf_static",):
        st = model.optimizer.state.get(getattr(model, n))
        if st is not None:
            out[n] = (float(st["step"]), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return out


def test_a_fused_model_pruned_by_the_kernels_equals_the_torch_path_bitwise():
    """Four direct fused steps at degree 0 and one degree bump (compact SH moments [P, 3, 3] beside the [P, 15, 3] parameter), then the same
    model pruned twice from one state: by the kernels and by the torch path.  Parameters, both moments, aggregated_mask and _mask_index
    are torch.equal; one more step from each ends equal too."""
    from das3r_amd import fast_step
    from das3r_amd.prune import NEVER_BLENDED, prune_points
    from das3r_amd.train import train_step
    model, cams, opt = _sequence_model(3, 32, 24, seed=9, fused=True)
    assert fast_step.available(model, PIPE)
    bg = torch.zeros(3, device="cuda")
    for it, u in enumerate([0, 2, 1, 0], start=1):
        train_step(model, cams[u], opt, it, PIPE, bg, fused=True)
    model.oneupSHdegree()
    with torch.no_grad():
        model._features_rest.copy_(0.05 * torch.randn(model._features_rest.shape, generator=torch.Generator().manual_seed(1)).cuda())
    train_step(model, cams[1], opt, 5, PIPE, bg, fused=True)
    assert tuple(model.optimizer.state[model._features_rest]["exp_avg"].shape)[1:] == (3, 3)
    P = model._xyz.shape[0]
    model.__dict__.pop("_fast_state", None)   # (per-model buffers of the direct iteration, rebuilt on demand: nothing to copy)
    a, b = copy.deepcopy(model), copy.deepcopy(model)
    ia = prune_points(a, min_opacity=NEVER_BLENDED)
    ib = prune_points(b, min_opacity=NEVER_BLENDED, use_kernels=False)
    assert ia["path"] == "kernels" and ib["path"] == "torch" and ia["after"] == ib["after"] and 0.6 * P < ia["after"] < 0.8 * P, (ia, ib)
    for n in PARAMS:
        assert torch.equal(getattr(a, n).detach(), getattr(b, n).detach()), n
        assert isinstance(getattr(a, n), torch.nn.Parameter) and getattr(a, n).shape[0] == ia["after"]
    ma, mb = _moments(a), _moments(b)
    assert set(ma) == set(mb) == set(PARAMS + ("_conf_static",))
    for n in ma:
        assert ma[n][0] == mb[n][0] == _moments(model)[n][0] and torch.equal(ma[n][1], mb[n][1]) and torch.equal(ma[n][2], mb[n][2]), n
    assert tuple(ma["_features_rest"][1].shape) == (ia["after"], 3, 3)
    assert torch.equal(a.aggregated_mask, b.aggregated_mask) and int(torch.count_nonzero(a.aggregated_mask)) == ia["after"]
    assert torch.equal(a._mask_index, b._mask_index) and torch.equal(a._mask_index, torch.nonzero(a.aggregated_mask.reshape(-1)).reshape(-1))
    assert "_fast_state" not in a.__dict__ and not hasattr(a._features_dc, "_das3r_mirror")
    la = train_step(a, cams[2], opt, 6, PIPE, bg, fused=True)[0]
    lb = train_step(b, cams[2], opt, 6, PIPE, bg, fused=True)[0]
    assert fast_step._state(a).P == ia["after"] and not fast_step._state(a).mask_is_everything
    assert abs(float(la) - float(lb)) <= util.GRAD_REL_TOL * abs(float(lb))


# ---------------------------------------------------------------------------------------------------------------- 4. 1/255 changes nothing
FORMS = {"torch-glue": dict(fused=False), "fused-autograd": dict(fused=True, fast_step=False), "fast-step": dict(fused=True, fast_step=True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_pruning_at_one_255th_changes_nothing_that_is_left(form):
    """A model with about 30 % of its Gaussians below 1/255 (conf_static == 0 / low raw opacity), and the same model pruned at 1/255.
    The forward images agree under assert_color_close; after ONE train step from identical state the loss, the survivors' updated
    parameters and the updated conf_static agree under assert_grad_close (GRAD_REL_TOL of the tensor's largest entry, no flip allowance);
    in the unpruned run the dropped rows got exactly zero gradient: their parameters did not move and their Adam moments are exactly 0."""
    from das3r_amd import fast_step
    from das3r_amd.prune import NEVER_BLENDED, prune_points
    from das3r_amd.render import das3r_render
    from das3r_amd.train import train_step
    fused = FORMS[form]["fused"]
    full, cams, opt = _sequence_model(3, 32, 24, seed=4, fused=fused)
    if "fast_step" in FORMS[form]:
        full.fast_step = FORMS[form]["fast_step"]
    assert (fused and fast_step.available(full, PIPE)) == (form == "fast-step")
    pruned = copy.deepcopy(full)
    P = full._xyz.shape[0]
    idx = torch.arange(P, device="cuda")
    eff = torch.sigmoid(full._opacity.detach()).reshape(-1) * full._conf_static.detach().reshape(-1)[idx]
    keep = ~(eff < torch.tensor(NEVER_BLENDED, dtype=torch.float32, device="cuda"))
    info = prune_points(pruned, min_opacity=NEVER_BLENDED)
    assert info["path"] == "kernels" and info["after"] == int(keep.sum()) and 0.25 * P < info["dropped"] < 0.35 * P, info
    bg = torch.zeros(3, device="cuda")
    uid = 1
    with torch.no_grad():
        img_full = das3r_render(cams[uid], full, PIPE, bg, camera_pose=full.get_RT(uid), fused=fused)["render"]
        img_pruned = das3r_render(cams[uid], pruned, PIPE, bg, camera_pose=pruned.get_RT(uid), fused=fused)["render"]
    d = float((img_full - img_pruned).abs().max())
    print(f"[{form}] P {P} -> {info['after']}; forward images: max |delta| {d:.3g}")
    util.assert_color_close(img_pruned.cpu().numpy(), img_full.cpu().numpy(), f"{form}: pruned vs unpruned image")
    before = {n: getattr(full, n).detach().clone() for n in PARAMS}
    l_full = float(train_step(full, cams[uid], opt, 1, PIPE, bg, fused=fused)[0])
    l_pruned = float(train_step(pruned, cams[uid], opt, 1, PIPE, bg, fused=fused)[0])
    torch.cuda.synchronize()
    print(f"[{form}] loss after one step: unpruned {l_full:.9g} pruned {l_pruned:.9g} (rel {abs(l_full - l_pruned) / abs(l_full):.3g})")
    assert abs(l_full - l_pruned) <= util.GRAD_REL_TOL * abs(l_full)
    moved = 0
    for n in PARAMS:
        a, b = getattr(pruned, n).detach(), getattr(full, n).detach()[keep]
        dev_ = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        print(f"[{form}] {n}: survivors' max |delta| / max|ref| = {dev_:.3g} (bar {util.GRAD_REL_TOL})")
        util.assert_grad_close(a.cpu().numpy(), b.cpu().numpy(), f"{form} {n}")
        # the dropped rows of the unpruned run: no gradient at all
        assert torch.equal(getattr(full, n).detach()[~keep], before[n][~keep]), f"{n}: a dropped row moved"
        st = full.optimizer.state.get(getattr(full, n))
        if st is not None and st["exp_avg"].shape[0] == P and st["exp_avg"].numel():
            assert float(st["exp_avg"][~keep].abs().max()) == 0.0 and float(st["exp_avg_sq"][~keep].abs().max()) == 0.0, f"{n}: a dropped row got a gradient"
        moved += int((getattr(full, n).detach()[keep] != before[n][keep]).sum())
    assert moved > 0, "the survivors were stepped"
    util.assert_grad_close(pruned._conf_static.detach().cpu().numpy(), full._conf_static.detach().cpu().numpy(), f"{form} conf_static")


# ---------------------------------------------------------------------------------------------------------------- 5. exact count at initialisation
def test_pruning_at_initialisation_drops_exactly_the_dynamic_pixels():
    from das3r_amd.prune import prune_points
    from das3r_amd.train import build_from_sequence, consistent_sequence, split_sequence
    seq = consistent_sequence(seed=0, moving=True, **SMALL)
    model, cams, _test = build_from_sequence(seq, heldout=True)
    tr, _ = split_sequence(seq)
    F = len(tr)
    assert F == len(cams) == model._conf_static.shape[0]
    dynamic = int((seq["dyna_avg"][torch.tensor(tr, device=seq["dyna_avg"].device)] == 1).sum())
    P = model._xyz.shape[0]
    assert dynamic > 0 and P == F * SMALL["W"] * SMALL["H"]
    info = prune_points(model, min_opacity=0.5 / F)
    assert info["path"] == "kernels" and info["before"] == P and info["dropped"] == dynamic and model._xyz.shape[0] == P - dynamic, (info, dynamic)
    assert int(torch.count_nonzero(model.aggregated_mask)) == P - dynamic
    assert bool((model._conf_static.detach().reshape(-1)[model._mask_index] == 1).all())


# ---------------------------------------------------------------------------------------------------------------- 6. a pruned job
PRUNE_JOB = dict(prune_from=100, prune_interval=100, prune_until=600, prune_min_opacity=0.005)


def _job(seed, iterations=600, **kw):
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.train import consistent_sequence
    seq = consistent_sequence(seed=seed, moving=True, **SMALL)
    keep = {}
    rec = run_sequence_job(seed, iterations, torch.device("cuda:0"), fused=True, seq=seq, keep=keep, **kw)
    return rec, keep[seed]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_pruned_job_finishes_reproduces_itself_and_keeps_its_heldout_psnr(seed):
    """consistent_sequence(seed, moving=True) at SMALL, held-out split, fused, 600 iterations, an event every 100 iterations from 100 at
    0.005.  Every render of the finished job is finite; it ends with fewer Gaussians than it began with; a second run ends bit-identical;
    its held-out static-region PSNR is not below BASELINE_PSNR[seed] (the unpruned job at the parent commit) by more than PSNR_MARGIN."""
    from das3r_amd.render import das3r_render
    assert PSNR_MARGIN is not None and BASELINE_PSNR[seed] is not None, "the parent commit's baselines have not been recorded (docs/ledger.md (cc))"
    rec, (model, cams, test_cams) = _job(seed, **PRUNE_JOB)
    assert rec["ok"] == 1 and np.isfinite(rec["psnr"])
    tr = [i for i in range(SMALL["frames"]) if (i + 5) % 10 != 0]
    P0 = len(tr) * SMALL["W"] * SMALL["H"]
    print(f"[pruned job seed {seed}] P {P0} -> {rec['n_splats']}; held-out static PSNR {rec['psnr']:.4f} dB (baseline {BASELINE_PSNR[seed]:.4f}, margin {PSNR_MARGIN:.3f})")
    assert rec["n_splats"] == model._xyz.shape[0] < P0
    assert int(torch.count_nonzero(model.aggregated_mask)) == rec["n_splats"]
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        for c in cams:
            assert bool(torch.isfinite(das3r_render(c, model, PIPE, bg, camera_pose=model.get_RT(c.uid), fused=True)["render"]).all())
        for c in test_cams:
            assert bool(torch.isfinite(das3r_render(c, model, PIPE, bg, camera_pose=model.get_RT_test(c.uid))["render"]).all())
    rec2, (model2, _c, _t) = _job(seed, **PRUNE_JOB)
    assert rec2["n_splats"] == rec["n_splats"] and rec2["psnr"] == rec["psnr"]
    for n in PARAMS + ("_conf_static", "Q", "T"):
        assert torch.equal(getattr(model, n).detach(), getattr(model2, n).detach()), f"{n}: a pruned job must reproduce itself bit for bit"
    assert rec["psnr"] >= BASELINE_PSNR[seed] - PSNR_MARGIN, (rec["psnr"], BASELINE_PSNR[seed], PSNR_MARGIN)


# ---------------------------------------------------------------------------------------------------------------- 7. resume
def test_a_pruned_job_resumes_bit_identical_and_refuses_another_threshold(tmp_path):
    """300 iterations, events after 100, 200 and 300, checkpoints every 150: the job killed after iteration 150 — behind its first event —
    and resumed ends with EQUAL parameters at the same size; the schedule is in the checkpoint's loop state, and resuming with another
    prune_min_opacity (or without pruning) raises ResumeMismatch."""
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.train import ResumeMismatch, consistent_sequence, latest_checkpoint
    dev = torch.device("cuda:0")
    seq = consistent_sequence(seed=5, moving=True, **SMALL)
    full_dir, res_dir, bad_dir = str(tmp_path / "full"), str(tmp_path / "resumed"), str(tmp_path / "other")
    keep_full, keep_res = {}, {}
    sched = dict(prune_from=100, prune_interval=100, prune_until=300, prune_min_opacity=0.005)
    kw = dict(fused=True, seq=seq, checkpoint_every=150, **sched)
    full = run_sequence_job(3, 300, dev, out_dir=full_dir, keep=keep_full, **kw)
    assert full["ok"] == 1 and latest_checkpoint(full_dir)[1] == 150
    extras = torch.load(os.path.join(full_dir, "chkpnt150.das3r.pth"), weights_only=False)
    assert tuple(extras["loop"]["prune"]) == (100, 100, 300, 0.005, 0.0)
    capture, _ = torch.load(os.path.join(full_dir, "chkpnt150.pth"), weights_only=False)
    P0 = int(seq["images"].shape[0] - 1) * SMALL["W"] * SMALL["H"]   # (12 frames: one held out)
    assert capture[1].shape[0] < P0, "the checkpoint was written behind the first event"
    assert int(torch.count_nonzero(extras["model"]["aggregated_mask"])) == capture[1].shape[0]
    for d in (res_dir, bad_dir):
        os.makedirs(d)
        for f in ("chkpnt150.pth", "chkpnt150.das3r.pth"):
            shutil.copy(os.path.join(full_dir, f), os.path.join(d, f))
    res = run_sequence_job(3, 300, dev, out_dir=res_dir, resume=True, keep=keep_res, **kw)
    assert res["ok"] == 1 and res["n_splats"] == full["n_splats"] < capture[1].shape[0]
    a, b = keep_full[3][0], keep_res[3][0]
    for n in PARAMS + ("_conf_static", "Q", "T"):
        assert torch.equal(getattr(a, n).detach(), getattr(b, n).detach()), f"{n}: a resumed pruned job must end bit-identical"
    assert torch.equal(a.aggregated_mask, b.aggregated_mask) and res["psnr"] == full["psnr"]
    with pytest.raises(ResumeMismatch, match="prun"):
        run_sequence_job(3, 300, dev, out_dir=bad_dir, resume=True, fused=True, seq=seq, checkpoint_every=150, **{**sched, "prune_min_opacity": 0.01})
    with pytest.raises(ResumeMismatch, match="prun"):
        run_sequence_job(3, 300, dev, out_dir=bad_dir, resume=True, fused=True, seq=seq, checkpoint_every=150)


# ---------------------------------------------------------------------------------------------------------------- 8. offline
@pytest.mark.parametrize("fused", [False, True])
def test_offline_renders_do_not_change_at_one_255th_and_the_pruned_ply_reloads(tmp_path, fused):
    from das3r_amd.farm import run_sequence_job
    from das3r_amd.io_formats import load_gaussians_ply
    from das3r_amd.offline import load_trained_model, render_sets
    from das3r_amd.prune import NEVER_BLENDED, prune_points
    from das3r_amd.train import consistent_sequence
    small = dict(SMALL, frames=6)
    seq = consistent_sequence(seed=2, moving=True, **small)
    out = str(tmp_path / "job")
    rec = run_sequence_job(0, 60, torch.device("cuda:0"), fused=True, seq=seq, out_dir=out)
    assert rec["ok"] == 1
    it, plain = render_sets(out, seq, write=False, fused=fused)
    it2, pruned = render_sets(out, seq, write=False, fused=fused, prune_min_opacity=NEVER_BLENDED, write_pruned_ply=True)
    assert it == it2 == 60 and len(plain) == len(pruned) == small["frames"]
    for k, (a, b) in enumerate(zip(pruned, plain)):
        util.assert_color_close(a.cpu().numpy(), b.cpu().numpy(), f"offline view {k} (fused={fused})")
    model, _ = load_trained_model(out, 60)
    P = model._xyz.shape[0]
    info = prune_points(model, min_opacity=NEVER_BLENDED)
    assert info["path"] == "kernels" and 0 < info["after"] < P
    g = load_gaussians_ply(os.path.join(out, "point_cloud", "iteration_60", "point_cloud_pruned.ply"))
    for name, attr in (("xyz", "_xyz"), ("features_dc", "_features_dc"), ("features_rest", "_features_rest"), ("opacity", "_opacity"),
                       ("conf_static", "_conf_static"), ("scaling", "_scaling"), ("rotation", "_rotation")):
        assert np.array_equal(g[name], getattr(model, attr).detach().cpu().numpy()), name
