"""CPU tests of voxel thinning (das3r_amd/thin.py, INTEGRATION.md "Voxel thinning"): the torch form of the rule against a brute-force
Python dict on hand-made inputs (floor not truncation, boundaries, ties, +-0 / NaN / +-inf scores, NaN / inf / out-of-range coordinates, no
score); the coverage opacity rule; create_from_frames without a thin option, and with an edge too small to merge anything, equals a
restatement of the initialisation bit for bit; the options of farm / offline, their mutual exclusion, and ResumeMismatch on a changed setting."""
import math
import random
import struct

import pytest
import torch

HALF = 1 << 20
NAN, INF = float("nan"), float("inf")


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _brute(xyz, score, inv_edge):
    """The rule of include/das3r_raster.h, point by point in Python floats rounded to fp32."""
    P = len(xyz)
    keep, count, cells = [True] * P, [1] * P, {}
    for i, p in enumerate(xyz):
        prod = [_f32(_f32(v) * _f32(inv_edge)) if math.isfinite(v) else v * inv_edge for v in p]
        if not all(math.isfinite(v) for v in prod):
            continue
        c = [math.floor(v) for v in prod]
        if not all(-HALF <= v < HALF for v in c):
            continue
        cells.setdefault(tuple(c), []).append(i)

    def better(a, b):   # does point a beat point b (a != b)?
        if score is None:
            return a < b
        sa, sb = score[a], score[b]
        if math.isnan(sa) or math.isnan(sb):
            return (not math.isnan(sa)) if math.isnan(sa) != math.isnan(sb) else a < b
        return sa > sb or (sa == sb and a < b)   # (-0.0 == 0.0 in Python as in IEEE)

    for members in cells.values():
        win = members[0]
        for m in members[1:]:
            if better(m, win):
                win = m
        for m in members:
            keep[m], count[m] = m == win, (len(members) if m == win else 0)
    return keep, count


def hand_made_cases():
    """(name, xyz rows, scores or None, inv_edge) — shared with the GPU test's layout (e)."""
    cases = []
    # a cell straddling zero: -0.3 and +0.3 are different cells at edge 1 (floor, not truncation); -0.0 lies in cell 0
    cases.append(("straddle", [[-0.3, 0, 0], [0.3, 0, 0], [-0.0, 0, 0], [0, -0.3, 0.3], [0, -1e-30, 0], [-1.0, 0, 0], [-0.999, 0, 0]],
                  [1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 3.0], 1.0))
    # points exactly on boundaries, at an edge whose inverse is exact (0.25) and one whose inverse is not (0.3)
    cases.append(("boundary", [[0.25, 0, 0], [0.2499999, 0, 0], [0.5, 0.25, 0], [0.49999997, 0.25, 0], [-0.25, 0, 0], [-0.25000003, 0, 0]],
                  [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], 4.0))
    cases.append(("boundary-inexact", [[0.3, 0, 0], [0.6, 0, 0], [0.90000004, 0, 0], [0.29999998, 0, 0], [-0.3, 0.3, 0.6]],
                  [1.0, 1.0, 1.0, 1.0, 1.0], _f32(1 / 0.3)))
    one = [[0.1 * k, 0.5, 0.5] for k in range(8)]
    cases.append(("ties", one, [2.0, 3.0, 3.0, 1.0, 3.0, 2.0, 0.5, 3.0], 1.0))
    cases.append(("zeros", one, [-0.0, 0.0, -1.0, -0.0, -5.0, -1e-40, -0.0, 0.0], 1.0))
    cases.append(("minus-zero-first", one[:3], [0.0, -0.0, 0.0][::-1], 1.0))
    cases.append(("nan-scores", one, [NAN, NAN, -INF, NAN, -INF, NAN, NAN, NAN], 1.0))
    cases.append(("all-nan", one[:4], [NAN, -NAN, NAN, NAN], 1.0))
    cases.append(("inf-scores", one, [1e38, INF, -INF, INF, NAN, 3.0, -3.0, 0.0], 1.0))
    cases.append(("neg-only", one[:5], [-3.0, -2.0, -INF, -2.0, NAN], 1.0))
    # coordinates that are not placeable never merge: NaN, +-inf, a product that overflows, cell 2^20 (out of range), cell -2^20 (in range)
    cases.append(("coords", [[NAN, 0, 0], [NAN, 0, 0], [0, INF, 0], [0, INF, 0], [0, 0, -INF], [3e38, 0, 0], [3e38, 0, 0],
                             [float(HALF), 0, 0], [float(HALF), 0, 0], [float(HALF) - 0.5, 0, 0], [float(HALF) - 0.25, 0, 0],
                             [-float(HALF), 0, 0], [-float(HALF) + 0.5, 0, 0], [-float(HALF) - 0.5, 0, 0], [-float(HALF) - 0.5, 0, 0],
                             [0.5, 0.5, 0.5], [0.25, 0.75, 0.5]],
                  [1.0] * 15 + [1.0, 2.0], 1.0))
    cases.append(("coords-scaled", [[3e20, 0, 0], [3e20, 0, 0], [2.0, 0, 0], [2.1, 0, 0]], [1.0, 1.0, 1.0, 2.0], 2e19))   # 3e20 * 2e19 overflows
    return cases


@pytest.mark.parametrize("with_score", [True, False])
@pytest.mark.parametrize("case", hand_made_cases(), ids=lambda c: c[0])
def test_torch_form_equals_a_brute_force_dict(case, with_score):
    from das3r_amd.thin import voxel_keep_torch
    _, xyz, score, inv_edge = case
    score = score if with_score else None
    keep, count = voxel_keep_torch(torch.tensor(xyz, dtype=torch.float32), None if score is None else torch.tensor(score, dtype=torch.float32), inv_edge)
    bk, bc = _brute(xyz, score, inv_edge)
    assert keep.dtype == torch.bool and count.dtype == torch.int32
    assert keep.tolist() == bk and count.tolist() == bc
    assert int(count.sum()) == len(xyz)   # every point is counted exactly once


def test_the_hand_made_cases_say_what_they_should():
    from das3r_amd.thin import voxel_keep_torch
    by = {c[0]: c for c in hand_made_cases()}
    run = lambda n, s=True: voxel_keep_torch(torch.tensor(by[n][1], dtype=torch.float32), torch.tensor(by[n][2], dtype=torch.float32) if s else None, by[n][3])
    keep, count = run("straddle")   # cells -1: {0, 5, 6}, 0: {1, 2}, (0,-1,0): {3, 4}
    assert keep.tolist() == [False, False, True, True, False, False, True] and count.tolist() == [0, 0, 2, 2, 0, 0, 3]
    keep, count = run("ties")       # the first of the 3.0s
    assert keep.tolist() == [False, True] + [False] * 6 and count[1] == 8
    keep, _ = run("zeros")          # -0 equals +0: index 0
    assert keep.tolist() == [True] + [False] * 7
    keep, _ = run("nan-scores")     # -inf beats NaN
    assert keep.tolist() == [False, False, True] + [False] * 5
    keep, _ = run("all-nan")
    assert keep.tolist() == [True, False, False, False]
    keep, count = run("coords")
    assert keep[:9].all() and (count[:9] == 1).all()            # not placeable: kept, count 1, never merged
    assert keep[9:11].tolist() == [True, False] and count[9] == 2   # cell 2^20 - 1 is in range
    assert keep[11:15].tolist() == [True, False, True, True] and count[11] == 2
    keep, _ = run("ties", False)    # no score: the lowest index
    assert keep.tolist() == [True] + [False] * 7


def test_random_clouds_against_the_dict():
    from das3r_amd.thin import inv_edge_of, voxel_keep_torch
    g = torch.Generator().manual_seed(5)
    xyz = (torch.rand(3000, 3, generator=g) - 0.5) * 6.0
    score = torch.randint(0, 5, (3000,), generator=g).float() - 2.0
    score[torch.rand(3000, generator=g) < 0.05] = NAN
    for edge in (0.3, 1.0, 7.0):
        inv = inv_edge_of(edge)
        assert inv == _f32(1.0 / edge)
        keep, count = voxel_keep_torch(xyz, score, inv)
        bk, bc = _brute(xyz.tolist(), score.tolist(), inv)
        assert keep.tolist() == bk and count.tolist() == bc
    for bad in (0.0, -1.0, NAN, INF, 1e-46):
        with pytest.raises(ValueError):
            inv_edge_of(bad)


def test_voxel_keep_off_device_takes_the_torch_form_and_true_is_refused():
    from das3r_amd.thin import inv_edge_of, voxel_keep, voxel_keep_torch
    xyz = torch.rand(200, 3, generator=torch.Generator().manual_seed(1))
    keep, count, kept = voxel_keep(xyz, None, edge=0.2)
    k2, c2 = voxel_keep_torch(xyz, None, inv_edge_of(0.2))
    assert torch.equal(keep, k2) and torch.equal(count, c2) and kept == int(k2.sum()) and 0 < kept < 200
    with pytest.raises(RuntimeError, match="HIP device"):
        voxel_keep(xyz, None, edge=0.2, use_kernels=True)
    with pytest.raises(ValueError):
        voxel_keep(xyz, None)


def test_pixel_footprint_is_the_median_of_depth_over_focal():
    from das3r_amd.thin import pixel_footprint
    depths = torch.tensor([[[1.0, 2.0], [3.0, 4.0]], [[10.0, 20.0], [30.0, NAN]]])
    K = torch.eye(3).repeat(2, 1, 1)
    K[0, 0, 0], K[1, 0, 0] = 2.0, 10.0
    assert pixel_footprint(depths, K, None) == 1.5           # {0.5, 1, 1.5, 2, 1, 2, 3}: torch's lower median
    mask = torch.tensor([[[True, False], [False, False]], [[False, False], [True, True]]])
    assert pixel_footprint(depths, K, mask) == 0.5           # {0.5, 3}
    with pytest.raises(ValueError):
        pixel_footprint(depths, K, torch.zeros(2, 2, 2, dtype=torch.bool))


@pytest.mark.parametrize("F", [2, 3, 7, 22, 50])
def test_coverage_opacity_rule(F):
    from das3r_amd.thin import COVERAGE_MAX, coverage_opacity
    count = torch.tensor([1, 2, 3, 1, F, 10 * F, 100000, 1], dtype=torch.int32)
    base = (1.0 / F) * torch.ones(count.numel(), 1)          # the parent's 1/F tensor
    out = coverage_opacity(count, base, F)
    assert out.dtype == torch.float32 and out.shape == base.shape
    ones = count == 1
    assert torch.equal(out[ones].view(torch.int32), base[ones].view(torch.int32))     # bitwise today's entry
    want = [min(1.0 - (1.0 - 1.0 / F) ** int(c), COVERAGE_MAX) for c in count.tolist()]
    got = out.reshape(-1).tolist()
    for c, w, v in zip(count.tolist(), want, got):
        if c != 1:
            assert v == _f32(w) or abs(v - w) <= 2 ** -23, (c, w, v)   # float64 pow of torch and of Python agree to fp32 rounding
    assert float(out.max()) <= _f32(COVERAGE_MAX) and float(out[6]) == _f32(COVERAGE_MAX)   # the clamp holds
    assert (out[~ones] > base[~ones]).all()


def _knn_torch(points):
    """Mean squared distance to the 3 nearest other points (what distCUDA2 computes; there is no CPU path of the kernel)."""
    d = torch.cdist(points.double(), points.double()) ** 2
    d.fill_diagonal_(float("inf"))
    return d.topk(3, largest=False).values.mean(dim=1).float()


def _tiny_sequence(F=3, H=12, W=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(F, 3, H, W, generator=g)
    depths = 4.0 + 0.5 * torch.rand(F, H, W, generator=g)
    confs = 0.2 * torch.randn(F, H, W, generator=g) + 0.3     # some pixels fall below log(conf_thre) = 0
    dyna = (torch.rand(F, H, W, generator=g) < 0.1).float()
    K = torch.tensor([[20.0, 0, W / 2], [0, 20.0, H / 2], [0, 0, 1.0]]).repeat(F, 1, 1)
    c2w = torch.eye(4).repeat(F, 1, 1)
    c2w[:, 0, 3] = 0.01 * torch.arange(F)
    pose7 = torch.cat([torch.tensor([[1.0, 0, 0, 0]]).repeat(F, 1), -c2w[:, :3, 3]], 1)
    return images, depths, confs, dyna, K, c2w, pose7


def _parent_init(images, depths, confs, dyna_avg, K, cam2world, sh_degree=3, conf_thre=1.0):
    """create_from_frames as it was before the thin options, restated."""
    from das3r_amd.losses import inverse_sigmoid, rgb_to_sh
    from das3r_amd.model import depth_to_points
    F = images.shape[0]
    pts = depth_to_points(K.float(), cam2world.float(), depths.float()).reshape(-1, 3)
    col = images.permute(0, 2, 3, 1).reshape(-1, 3)
    mask = confs.reshape(-1) > torch.tensor(conf_thre).log()
    pts, col = pts[mask].contiguous(), col[mask]
    n = pts.shape[0]
    feats = torch.zeros(n, 3, (sh_degree + 1) ** 2)
    feats[:, :3, 0] = rgb_to_sh(col)
    scales = torch.log(torch.sqrt(torch.clamp_min(_knn_torch(pts), 0.0000001)))[..., None].repeat(1, 3)
    rots = torch.zeros(n, 4)
    rots[:, 0] = 1
    opac = inverse_sigmoid((1.0 / F) * torch.ones(n, 1))
    return dict(aggregated_mask=mask, _xyz=pts, _features_dc=feats[:, :, 0:1].transpose(1, 2).contiguous(),
                _features_rest=feats[:, :, 1:].transpose(1, 2).contiguous(), _scaling=scales, _rotation=rots, _opacity=opac,
                _conf_static=(1 - dyna_avg.float()).contiguous())


def _bits_equal(a, b):
    a, b = a.detach(), b.detach()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_create_from_frames_without_thinning_and_with_a_tiny_edge_equals_the_parent(monkeypatch):
    from das3r_amd import model as M
    monkeypatch.setattr(M, "distCUDA2", _knn_torch)
    seq = _tiny_sequence()
    want = _parent_init(*seq[:6])
    assert 0 < int(want["aggregated_mask"].sum()) < want["aggregated_mask"].numel()
    plain = M.SplatModel(3).create_from_frames(*seq)
    assert plain.thin_info is None and plain.thin_init is None
    for kw in (dict(thin_edge=1e-6), dict(thin_relative=1e-5), dict(thin_edge=1e-6, thin_opacity="reference")):
        tiny = M.SplatModel(3).create_from_frames(*seq, **kw)
        assert tiny.thin_info["before"] == tiny.thin_info["after"] == want["_xyz"].shape[0]
        for m in (plain, tiny):
            for k, v in want.items():
                assert _bits_equal(getattr(m, k), v), (kw, k)
    with pytest.raises(ValueError, match="not both"):
        M.SplatModel(3).create_from_frames(*seq, thin_edge=0.1, thin_relative=1.0)
    with pytest.raises(ValueError, match="thin_opacity"):
        M.SplatModel(3).create_from_frames(*seq, thin_edge=0.1, thin_opacity="other")


@pytest.mark.parametrize("mode", ["coverage", "reference"])
def test_create_from_frames_thinned_follows_the_rule(monkeypatch, mode):
    from das3r_amd import model as M
    from das3r_amd import thin
    from das3r_amd.losses import inverse_sigmoid
    monkeypatch.setattr(M, "distCUDA2", _knn_torch)
    seq = _tiny_sequence(seed=2)
    images, depths, confs, dyna, K, c2w, _ = seq
    want = _parent_init(*seq[:6])
    fp = thin.pixel_footprint(depths, K, want["aggregated_mask"])
    m = M.SplatModel(3).create_from_frames(*seq, thin_relative=2.0, thin_opacity=mode)
    assert m.thin_init == ("relative", 2.0, mode) and m.thin_info["edge"] == 2.0 * fp
    keep, count = thin.voxel_keep_torch(want["_xyz"], confs.reshape(-1)[want["aggregated_mask"]].float(), thin.inv_edge_of(2.0 * fp))
    assert 0 < int(keep.sum()) < keep.numel() and m._xyz.shape[0] == int(keep.sum()) == m.thin_info["after"]
    pixels = torch.nonzero(want["aggregated_mask"]).reshape(-1)
    mask = torch.zeros_like(want["aggregated_mask"])
    mask[pixels[keep]] = True
    assert torch.equal(m.aggregated_mask, mask)                       # the cleared bits are exactly the losers
    assert _bits_equal(m._xyz, want["_xyz"][keep]) and _bits_equal(m._features_dc, want["_features_dc"][keep])
    scales = torch.log(torch.sqrt(torch.clamp_min(_knn_torch(want["_xyz"][keep]), 0.0000001)))[..., None].repeat(1, 3)
    assert _bits_equal(m._scaling, scales)                            # the k-NN of the survivors only
    F = images.shape[0]
    base = (1.0 / F) * torch.ones(int(keep.sum()), 1)
    opac = base if mode == "reference" else thin.coverage_opacity(count[keep], base, F)
    assert _bits_equal(m._opacity, inverse_sigmoid(opac))
    if mode == "coverage":
        assert (count[keep] > 1).any() and (torch.sigmoid(m._opacity.detach()) <= 0.99 + 1e-6).all()
    assert _bits_equal(m._conf_static, want["_conf_static"])           # per pixel: stays


def test_thin_model_on_a_host_model_is_prune_points_with_the_losers(monkeypatch):
    from das3r_amd import thin
    from das3r_amd.model import OptimParams
    from tests.test_prune_host import PARAMS, _host_model
    a, b = _host_model(seed=3), _host_model(seed=3)
    for m in (a, b):
        m.training_setup(OptimParams())
    score = thin.default_score(a)
    idx = torch.nonzero(a.aggregated_mask.reshape(-1)).reshape(-1)
    assert torch.equal(score, torch.sigmoid(a._opacity.detach()).reshape(-1) * a._conf_static.detach().reshape(-1)[idx])
    keep, _, kept = thin.voxel_keep(a._xyz.detach(), score, edge=0.8)
    info = thin.thin_model(a, 0.8)
    drop0 = (score < 0).sum().item()   # prune_points(min_opacity=0) also drops what renders with a negative opacity
    assert info["edge"] == 0.8 and info["path"] == "torch" and info["before"] == b._xyz.shape[0] and 0 < info["after"] <= kept
    from das3r_amd.prune import prune_points
    prune_points(b, min_opacity=0.0, also_drop=~keep)
    assert info["after"] == b._xyz.shape[0] >= kept - drop0
    for n in PARAMS:
        assert _bits_equal(getattr(a, n), getattr(b, n))
    assert torch.equal(a.aggregated_mask, b.aggregated_mask) and torch.equal(a._mask_index, b._mask_index)


def test_the_options_are_off_by_default_and_exclusive():
    from das3r_amd import farm, offline
    from das3r_amd.model import OptimParams
    from das3r_amd.train import thin_settings
    assert OptimParams().prune_thin_edge == 0.0
    args = farm.parser().parse_args([])
    assert (args.thin_init_relative, args.thin_init_edge, args.thin_opacity, args.prune_thin_relative) == (None, None, "coverage", None)
    assert farm.thin_kwargs(args) == {}                        # off: run_sequence_job is called as it was
    args = farm.parser().parse_args("--thin-init-relative 1.5 --thin-opacity reference".split())
    assert farm.thin_kwargs(args) == dict(thin_init_relative=1.5, thin_init_edge=None, thin_opacity="reference", prune_thin_relative=None)
    args = farm.parser().parse_args("--thin-init-edge 0.02 --prune-thin-relative 2 --prune-from 10 --prune-interval 10 --prune-until 50".split())
    assert farm.thin_kwargs(args) == dict(thin_init_relative=None, thin_init_edge=0.02, thin_opacity="coverage", prune_thin_relative=2.0)
    with pytest.raises(SystemExit):
        farm.parser().parse_args("--thin-init-edge 0.02 --thin-init-relative 1".split())
    with pytest.raises(SystemExit):
        farm.parser().parse_args("--thin-opacity other".split())
    with pytest.raises(SystemExit):                            # thinning at the prune events needs prune events
        farm.thin_kwargs(farm.parser().parse_args("--prune-thin-relative 2".split()))
    a = offline.parser().parse_args(["-m", "x", "-s", "y"])
    assert a.thin_edge is None and a.thin_relative is None
    a = offline.parser().parse_args(["-m", "x", "-s", "y", "--thin-relative", "1.0", "--write-pruned-ply"])
    assert a.thin_relative == 1.0 and a.write_pruned_ply
    with pytest.raises(SystemExit):
        offline.parser().parse_args(["-m", "x", "-s", "y", "--thin-edge", "0.1", "--thin-relative", "1.0"])
    with pytest.raises(ValueError, match="not both"):
        offline.render_sets("nowhere", {}, thin_edge=0.1, thin_relative=1.0)
    plain = type("M", (), {})()
    assert thin_settings(plain, OptimParams()) is None
    plain.thin_init = ("relative", 1.0, "coverage")
    assert thin_settings(plain, OptimParams(prune_thin_edge=0.25)) == (("relative", 1.0, "coverage"), 0.25)


class _Stop(Exception):
    pass


def test_resume_with_other_thin_settings_is_refused(monkeypatch):
    from das3r_amd import train as T
    from das3r_amd.model import OptimParams
    from tests.test_prune_host import _host_model
    model = _host_model()
    model.training_setup(OptimParams())
    cams = [type("Cam", (), {"uid": u})() for u in range(3)]
    sched = dict(prune_from_iter=100, prune_interval=100, prune_until_iter=600)
    base = dict(rng=random.Random(0).getstate(), stack=[0, 1], ema=torch.zeros(()), last_psnr=torch.zeros(()), library=None, depth_l1=(0.0, 0.0))

    def stop(*a, **k):
        raise _Stop()

    monkeypatch.setattr(T, "train_step", stop)
    saved = {}
    monkeypatch.setattr(T, "save_checkpoint", lambda path, m, it, loop_state=None: saved.update(loop=loop_state))
    # what a thinned job writes into its checkpoints
    model.thin_init = ("relative", 1.0, "coverage")
    monkeypatch.setattr(T, "train_step", lambda *a, **k: (torch.zeros(()), torch.zeros(()), None))
    T.train(model, cams, OptimParams(), 4, checkpoint_every=2, checkpoint_dir="unused")
    assert saved["loop"]["thin"] == (("relative", 1.0, "coverage"), 0.0)
    monkeypatch.setattr(T, "train_step", stop)
    loop = dict(base, thin=saved["loop"]["thin"])
    with pytest.raises(_Stop):   # the same settings pass the check (and reach the first step)
        T.train(model, cams, OptimParams(), 10, start_iteration=5, loop_state=dict(loop))
    for init, opt in ((("relative", 2.0, "coverage"), OptimParams()), (("relative", 1.0, "reference"), OptimParams()), (("edge", 1.0, "coverage"), OptimParams()),
                      (None, OptimParams()), (("relative", 1.0, "coverage"), OptimParams(prune_thin_edge=0.1, **sched))):
        model.thin_init = init
        with pytest.raises(T.ResumeMismatch, match="thin"):
            T.train(model, cams, opt, 10, start_iteration=5, loop_state=dict(loop, prune=(100, 100, 600, 0.005, 0.0)) if opt.prune_interval else dict(loop))
    # a checkpoint from before thinning: off
    model.thin_init = None
    with pytest.raises(_Stop):
        T.train(model, cams, OptimParams(), 10, start_iteration=5, loop_state=dict(base))
    assert "thin" not in base
    model.thin_init = ("edge", 0.5, "coverage")
    with pytest.raises(T.ResumeMismatch, match="thin"):
        T.train(model, cams, OptimParams(), 10, start_iteration=5, loop_state=dict(base))
    # the prune events' edge
    model.thin_init = None
    loop = dict(base, prune=(100, 100, 600, 0.005, 0.0), thin=(None, 0.25))
    with pytest.raises(_Stop):
        T.train(model, cams, OptimParams(prune_thin_edge=0.25, **sched), 10, start_iteration=5, loop_state=dict(loop))
    for other in (OptimParams(prune_thin_edge=0.5, **sched), OptimParams(**sched)):
        with pytest.raises(T.ResumeMismatch, match="thin"):
            T.train(model, cams, other, 10, start_iteration=5, loop_state=dict(loop))
    with pytest.raises(ValueError, match="schedule is off"):
        T.train(model, cams, OptimParams(prune_thin_edge=0.25), 10)


def test_train_passes_the_voxel_losers_to_the_prune_events(monkeypatch):
    from das3r_amd import prune as PR
    from das3r_amd import thin
    from das3r_amd import train as T
    from das3r_amd.model import OptimParams
    from tests.test_prune_host import _host_model
    model = _host_model()
    model.training_setup(OptimParams())
    cams = [type("Cam", (), {"uid": u})() for u in range(3)]
    events = []
    monkeypatch.setattr(T, "train_step", lambda *a, **k: (torch.zeros(()), torch.zeros(()), None))
    monkeypatch.setattr(PR, "prune_points", lambda m, **k: events.append(k))
    T.train(model, cams, OptimParams(prune_from_iter=2, prune_interval=2, prune_until_iter=4, prune_thin_edge=0.8), 5)
    keep, _, _ = thin.voxel_keep(model._xyz.detach(), thin.default_score(model), edge=0.8)
    assert len(events) == 2 and 0 < int(keep.sum()) < keep.numel()
    for k in events:
        assert k["min_opacity"] == 0.005 and k["max_world_scale"] == 0.0 and torch.equal(k["also_drop"], ~keep)
    events.clear()
    T.train(model, cams, OptimParams(prune_from_iter=2, prune_interval=2, prune_until_iter=4), 5)
    assert events == [dict(min_opacity=0.005, max_world_scale=0.0)] * 2   # off: the call as it was
