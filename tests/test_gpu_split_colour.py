"""GPU tests of the split preprocess (preprocess.hip: preprocess_geometry_kernel on the caller's stream, sh_colour_kernel on the library's
side stream beside the binning kernels, joined in front of the compositing forward): with DAS3R_SPLIT_COLOUR=1 every byte a forward leaves
and every gradient its backward computes is the byte DAS3R_SPLIT_COLOUR=0 (the fused preprocess_kernel) gives — the geometry buffer's
records, `clamped`, the nine Jacobian planes, radii, num_rendered, the image(s) — for SH degree 1 - 3 in every form of the call, on the
redo path, and with two jobs in flight on two caller streams.  Which kernels ran is read from the library's own launch record."""

import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

SHJAC = 4   # das3r_raster_saved.flags bit 2
GRADS = ["means2D", "colors", "opacities", "means3D", "cov3D", "shs", "scales", "rotations"]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _scene(D, M, P=3000, W=128, H=80, seed=70, s_px=(0.5, 4.0)):
    from das3r_amd.synth import make_scene
    sc = make_scene(P=P, W=W, H=H, focal=100.0 * W / 128, sh_degree=D, seed=seed + D, bg=(0.1, 0.2, 0.3), s_px=s_px)
    sc.shs[: sc.P // 5, 0, :2] = -3.0          # two channels clamped at 0 for a fifth of the splats
    sc.means3D[sc.P // 2: sc.P // 2 + 40, 2] = -1.0   # forty splats behind the camera: culled records stay zero in either form
    sc.shs = sc.shs[:, :M].contiguous()
    return sc


def _pre(sc, dev, keep):
    """The raw-parameter form (das3r_raster_in.pre) of the same scene: identity pose, log scales, opacity logits with confidence 1."""
    from das3r_amd import _lib
    xyz, rot = sc.means3D.to(dev), sc.rotations.to(dev)
    scaling = torch.log(sc.scales).to(dev)
    op = sc.opacities.clamp(1e-4, 1 - 1e-4)
    logit = torch.log(op / (1 - op)).to(dev)
    conf = torch.ones(sc.P, device=dev)
    mats = torch.zeros(28, device=dev)
    mats[[0, 4, 8]] = 1.0
    mats[[12, 17, 22, 27]] = 1.0
    keep += [xyz, rot, scaling, logit, conf, mats]
    pre = _lib.PreTransform()
    pre.xyz, pre.rot, pre.scaling, pre.opacity_raw = xyz.data_ptr(), rot.data_ptr(), scaling.data_ptr(), logit.data_ptr()
    pre.conf_flat, pre.mask_index = conf.data_ptr(), None
    pre.R, pre.t, pre.Lq = mats.data_ptr(), mats.data_ptr() + 36, mats.data_ptr() + 48
    return pre


def _kernels(report):
    return {k for k in report if k.startswith("preprocess") or k.startswith("sh_colour")}


def _forward_backward(sc, dev, form="plain", exact=True, no_backward=False, colors=False):
    """One forward (+ backward) of `sc`; -> dict of everything the two forms are compared on, and the per-Gaussian kernels that ran."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    e = torch.empty(0, device=dev)
    rs = GaussianRasterizationSettings(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.settings_kwargs().items()})
    means3D, opac = sc.means3D.to(dev), sc.opacities.to(dev)
    shs = e if colors else sc.shs.to(dev)
    cols = torch.rand(sc.P, 3, generator=torch.Generator().manual_seed(9)).to(dev) if colors else e
    cov = form == "cov"
    scales, rot = (e, e) if cov else (sc.scales.to(dev), sc.rotations.to(dev))
    cov3D = util.cov3d_of(sc).to(dev) if cov else e
    keep = []
    pre = _pre(sc, dev, keep) if form == "pre" else None
    depth = form == "depth"
    _lib.profile_enable(True)
    try:
        fw = rasterizer._forward_full(rs, means3D, shs, cols, opac, scales, rot, cov3D, exact=exact, pre=pre, invdepth=depth,
                                      no_backward=no_backward, antialiasing=form == "aa")
        torch.cuda.synchronize()
        ran = _kernels(_lib.profile_report())
    finally:
        _lib.profile_enable(False)
    I, color, radii, geom, binning, img, cap = fw[:7]
    L = _lib.layout(sc.P, int(cap), sc.W, sc.H)
    out = {"num_rendered": int(I), "capacity": int(cap), "flags": int(cap.flags), "color": color.clone(), "radii": radii.clone(),
           "records": geom[L["xy"]: L["xy"] + 64 * sc.P].clone(), "clamped": geom[L["clamped"]: L["clamped"] + sc.P].clone()}
    if depth:
        out["invdepth"] = fw[7].clone()
    if cap.flags & SHJAC:
        off = _lib.layout(sc.P, 0, sc.W, sc.H)["geom_bytes"]
        out["planes"] = geom[off: off + 36 * sc.P].clone()
    if not no_backward:
        dD = torch.randn(1, sc.H, sc.W, generator=torch.Generator().manual_seed(5)).to(dev) / (sc.W * sc.H) if depth else None
        g = rasterizer._backward_impl(rs, I, sc.dL_dpix.to(dev), means3D, shs, cols, opac, scales, rot, cov3D, geom, binning, img, cap,
                                      pre=pre, grad_invdepth=dD)
        torch.cuda.synchronize()
        for name, t in zip(GRADS, g):
            if t is not None:
                out["grad_" + name] = t.clone()
    assert keep is not None
    return out, ran


def _assert_same(a, b, what):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs between the split and the fused preprocess"
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _both(monkeypatch, run):
    """run() with the split forced off, then on; -> (fused result, split result) after checking which kernels each launched."""
    from das3r_amd import _lib
    res = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("DAS3R_SPLIT_COLOUR", sw)
        _lib.forget_shapes()   # (both runs start from the same learnt state: a shape's first forward)
        res[sw] = run()
    assert res["0"][1] == {"preprocess_kernel"}, res["0"][1]
    assert res["1"][1] == {"preprocess_geometry_kernel", "sh_colour_kernel"}, res["1"][1]
    return res["0"][0], res["1"][0]


FORMS = ("plain", "aa", "pre", "depth", "cov")
# every degree x form on the local order; the segmented path (the other binning chain the split form runs beside) with the staged and
# the unstaged rows in three forms
CASES = [(D, M, form, "local") for D, M in ((1, 4), (1, 16), (2, 9), (2, 16), (3, 16)) for form in FORMS] + \
        [(1, 16, "plain", "seg"), (2, 9, "pre", "seg"), (2, 16, "plain", "seg"), (3, 16, "plain", "seg"), (3, 16, "depth", "seg")]


@pytest.mark.parametrize("D,M,form,binning", CASES)
def test_split_forward_and_backward_are_bit_identical_to_the_fused_kernel(monkeypatch, D, M, form, binning):
    dev = _dev()
    monkeypatch.setenv("DAS3R_BINNING", binning)       # a binning chain of its own: the paths the split form runs on
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")     # (gradients comparable bit for bit run to run)
    sc = _scene(D, M)
    fused, split = _both(monkeypatch, lambda: _forward_backward(sc, dev, form))
    assert fused["num_rendered"] > 0 and bool(fused["flags"] & SHJAC) == (D >= 2)
    assert ("planes" in split) == (D >= 2)
    rec = fused["records"].view(torch.float32).view(sc.P, 16)
    assert (rec[:, 8:11].abs().sum(1) > 0).sum() > sc.P // 2, "the records carry colours"
    assert (fused["radii"] == 0).sum() >= 40 and fused["clamped"].any()
    _assert_same(fused, split, f"D{D} M{M} {form} {binning}")


@pytest.mark.parametrize("D", [2, 3])
def test_a_forward_no_backward_follows_writes_no_planes_in_either_form(monkeypatch, D):
    dev = _dev()
    monkeypatch.setenv("DAS3R_BINNING", "local")
    sc = _scene(D, 16)
    fused, split = _both(monkeypatch, lambda: _forward_backward(sc, dev, no_backward=True))
    assert not fused["flags"] & SHJAC and not split["flags"] & SHJAC and "planes" not in split
    _assert_same(fused, split, f"D{D} no backward")
    monkeypatch.setenv("DAS3R_SPLIT_COLOUR", "1")
    train, _ = _forward_backward(sc, dev)
    assert train["flags"] & SHJAC and torch.equal(train["color"], split["color"]) and torch.equal(train["records"], split["records"])


def test_the_redo_after_a_capacity_overflow_is_bit_identical(monkeypatch):
    """The speculative layout (capacity from the shape's previous forward) overflows when the scene grows: binning and compositing are redone
    with the exact size, the colours of the first pass stay.  Same bits as the fused kernel through the same redo."""
    from das3r_amd import _lib
    dev = _dev()
    monkeypatch.setenv("DAS3R_BINNING", "local")
    monkeypatch.setenv("DAS3R_FUSED_EMIT", "0")        # (a scene this small would otherwise emit inside the preprocess kernel)
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    small = _scene(3, 16, P=4000, W=256, H=160, seed=80, s_px=(0.3, 1.0))
    grown = _scene(3, 16, P=4000, W=256, H=160, seed=80, s_px=(6.0, 12.0))

    def run():
        first, ran1 = _forward_backward(small, dev, exact=False)
        second, ran2 = _forward_backward(grown, dev, exact=False)
        assert ran1 == ran2
        # the premise: the second forward's count is beyond the headroom of the first (25 % + 4096), and its buffer was laid out again, exactly
        assert second["num_rendered"] > first["num_rendered"] * 5 // 4 + 4096 and second["capacity"] == second["num_rendered"]
        return second, ran2

    fused, split = _both(monkeypatch, run)
    _assert_same(fused, split, "redo")
    # the speculative path without an overflow, for completeness: the same scene twice
    again = _both(monkeypatch, lambda: (_forward_backward(small, dev, exact=False), _forward_backward(small, dev, exact=False))[1])
    assert again[0]["capacity"] > again[0]["num_rendered"]
    _assert_same(*again, "speculative")
    _lib.forget_shapes()


def test_degree_0_and_precomputed_colours_take_the_fused_kernel(monkeypatch):
    dev = _dev()
    monkeypatch.setenv("DAS3R_BINNING", "local")
    monkeypatch.setenv("DAS3R_SPLIT_COLOUR", "1")
    for M in (1, 16):
        _, ran = _forward_backward(_scene(0, M), dev)
        assert ran == {"preprocess_kernel"}, (M, ran)
    _, ran = _forward_backward(_scene(3, 16), dev, colors=True)
    assert ran == {"preprocess_kernel"}, ran
    monkeypatch.setenv("DAS3R_BINNING", "radix")       # the global depth sort scatters the depth keys: fused, whatever the switch says
    _, ran = _forward_backward(_scene(3, 16), dev)
    assert ran == {"preprocess_kernel"}, ran
    monkeypatch.setenv("DAS3R_BINNING", "local")
    _, ran = _forward_backward(_scene(3, 16), dev)
    assert ran == {"preprocess_geometry_kernel", "sh_colour_kernel"}, ran


def test_two_jobs_in_flight_on_two_streams_reproduce_their_solo_results(monkeypatch):
    """Two host threads, each with its own stream (farm.run_jobs), each rendering its own scene forwards and backwards with the split on: every
    job has a side stream of its own beside its caller stream, and ends with the bits it ends with alone."""
    from das3r_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib
    from das3r_amd.farm import run_jobs
    dev = _dev()
    monkeypatch.setenv("DAS3R_SPLIT_COLOUR", "1")
    monkeypatch.setenv("DAS3R_FUSED_EMIT", "0")
    monkeypatch.setenv("DAS3R_BINNING", "local")
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    scenes = [_scene(3, 16, P=20000, W=256, H=160, seed=90 + 7 * s).to(dev) for s in range(2)]

    def job(s):
        sc = scenes[s]
        _lib.forget_shapes()
        rs = GaussianRasterizationSettings(**sc.settings_kwargs())
        leaves = {k: getattr(sc, k).clone().requires_grad_() for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        means2D = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
        rast = GaussianRasterizer(rs)
        colors = []
        for it in range(12):
            for t in leaves.values():
                t.grad = None
            color, radii = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"],
                                scales=leaves["scales"], rotations=leaves["rotations"])
            color.backward(sc.dL_dpix)
            with torch.no_grad():
                leaves["shs"].add_(leaves["shs"].grad, alpha=-0.05)   # (the scene changes from step to step, through the colour path)
            colors.append(color.detach().clone())
        torch.cuda.current_stream().synchronize()
        return colors + [radii.clone()] + [t.grad.clone() for t in leaves.values()] + [leaves["shs"].detach().clone()]

    solo = [job(s) for s in range(2)]
    again = job(0)
    assert all(torch.equal(a, b) for a, b in zip(solo[0], again)), "a job run twice alone must reproduce itself bit for bit"
    duo = run_jobs(range(2), job, 2, dev)
    torch.cuda.synchronize()
    for s in range(2):
        assert len(solo[s]) == len(duo[s])
        for k, (a, b) in enumerate(zip(solo[s], duo[s])):
            assert torch.equal(a, b), (s, k)
    assert not torch.equal(solo[0][0], solo[1][0]), "the two scenes are meant to be different jobs"
    _lib.forget_shapes()
