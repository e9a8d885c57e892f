"""Guard bands and poison round every buffer the rasterizer's Python layer hands the library (tests/guard_bands.py): the allocator callbacks'
geom / binning / img, colour, radii and inverse depth, the scratch buffers (also 4-, 8- and 12-byte misaligned), the gradient sets, the
focal workspace, and the outputs and scratch of the saved-list calls.  The sizes are the library's own arithmetic (the *_bytes functions,
the three sizes the forward asks its callbacks for); nothing else looks at what a kernel writes past them.

Every case runs its operation once as the product allocates and once under guarded(pattern) for 0x00, 0xFF and the NaN word: the bands must
be intact, and every output the same bits in all four runs — a changed band is a store outside a buffer, a changed result a read of memory
the library never wrote.  das3r_raster_forget_shapes comes before every forward, so the four runs take the same plan; the gradients are
compared under DAS3R_DETERMINISTIC=1 (fixed summation order), except where a case says otherwise.  The tests of the workspace entries
(knn, thin, prune, mesh, tsdf, losses, pose) are in tests/test_gpu_guard_bands_workspaces.py."""
import pytest
import torch

from tests import util
from tests.guard_bands import assert_same_bits, four_runs
from tests.test_gpu_bucket_local import GRADS, _dev, _view
from tests.test_gpu_cell_sort import _scene as cell_scene, run as cell_run

pytestmark = pytest.mark.gpu

ALLOC_SITE = "rasterizer.py"   # (the call sites the messages name are the Python layer's own lines)


# ---------------------------------------------------------------------------------------------------------------- the driver
_INPUTS = {}


def _inputs(name, scene=None):
    """(scene, settings keywords, the seven input tensors of _forward_full, dL/dcolour, dL/dinvdepth) of a util.scene_variant — or of
    scene = (Scene, mode) under the key `name` — on the device: made once, never written"""
    if name not in _INPUTS:
        dev = _dev()
        sc, mode = util.scene_variant(name) if scene is None else scene
        kw = {k: v.to(dev) for k, v in util.raster_inputs(sc, mode).items()}
        skw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in util.settings_kwargs(sc, mode).items()}
        e = torch.empty(0, device=dev)
        args = (kw["means3D"], kw.get("shs", e), kw.get("colors_precomp", e), kw["opacities"], kw.get("scales", e), kw.get("rotations", e),
                kw.get("cov3D_precomp", e))
        _INPUTS[name] = (sc, skw, args, sc.dL_dpix.to(dev), (torch.randn(1, sc.H, sc.W, generator=torch.Generator().manual_seed(5)) * 0.5).to(dev))
    return _INPUTS[name]


def drive(name, before=(), exact=True, invdepth=False, antialiasing=False, backward=True, misaligns=(0,), focal=False, profile=False,
          inputs=None):
    """das3r_raster_forget_shapes, the forwards of `before` (scale modifiers), one forward and its backward per entry of `misaligns` -> all a
    forward and a backward leave behind (on the host), with the launch table when `profile`."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    sc, skw, args, dL, dD = inputs if inputs is not None else _inputs(name)

    def forward(mod):
        rs = GaussianRasterizationSettings(**{**skw, "scale_modifier": mod * skw["scale_modifier"]})
        return rs, rasterizer._forward_full(rs, *args, exact=exact, invdepth=invdepth, antialiasing=antialiasing)

    _lib.forget_shapes()
    for mod in before:
        forward(mod)
    torch.cuda.synchronize()
    _lib.profile_report()
    _lib.profile_enable(profile)
    try:
        rs, out = forward(1.0)
        I, color, radii, geom, binning, img, cap = out[:7]
        grads = []
        for off in misaligns if backward else ():
            g = rasterizer._backward_impl(rs, I, dL, *args, geom, binning, img, cap, _scratch_misalign=off, grad_invdepth=dD if invdepth else None,
                                          **(dict(focal=True, focal_per_splat=True) if focal else {}))
            names = GRADS + (("focal_sums", "focal_per_splat") if focal else ())
            grads.append({k: t.cpu() for k, t in zip(names, g) if t is not None})
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    ran = {k: n for k, (n, _ms) in _lib.profile_report(raw=True).items()} if profile else None
    res = dict(I=int(I), cap=int(cap), color=color.cpu(), radii=radii.cpu(), grads=grads)
    if sc.P > 0 and int(cap) > 0:
        L = _lib.layout(sc.P, int(cap), sc.W, sc.H)
        npix, tiles = sc.W * sc.H, ((sc.W + 15) // 16) * ((sc.H + 15) // 16)
        res.update(point_list=_view(binning, L["point_list"], torch.int32, int(I)).cpu(), ranges=_view(img, L["ranges"], torch.int32, 2 * tiles).cpu(),
                   final_T=_view(img, L["final_T"], torch.int32, npix).cpu(), n_contrib=_view(img, L["n_contrib"], torch.int32, npix).cpu())
    if invdepth:
        res["invdepth"] = out[7].cpu()
    return res, ran


def _without(res, *keys):
    return {k: v for k, v in res.items() if k not in keys}


# ------------------------------------------------------------------------------------------- forward: every binning plan, every capacity regime
PLANS = ("", "radix", "local", "seg", "seg3", "bucket", "cells")   # "": DAS3R_BINNING unset — by shape (32 tiles, 1200 splats: the local order)
REGIMES = {"exact": dict(exact=True), "fits": dict(exact=False, before=(1.0,)), "overflow": dict(exact=False, before=(0.15,))}
SPECULATING = ("", "local", "seg", "seg3", "bucket", "cells")


def launches(ran, prefix):
    return sum(n for k, n in ran.items() if k.startswith(prefix))


def assert_plan_ran(plan, ran, binnings, speculative):
    """From the profiler's kernel names: the plan ran, `binnings` times (2: clamped, then redone).  What tells the plans apart:
    depth_hist_kernel is the global sort's, segment_sort_kernel the segmented path's (seg3: one more partition pass than the 32 tiles need),
    cell_finish_kernel the cells plan's.  The bucket plan and the local order both end in tile_ranges_kernel with none of the three, and a
    forward laid out exactly launches the same names under both; a speculative one does not: the local order's emission then runs inside the
    preprocess kernel (no scan_emit_kernel until a redo), the bucket plan's carries depth buckets and keeps its scan_emit_kernel."""
    sort, seg, cell, ranges, emit = (launches(ran, k) for k in ("depth_hist_kernel", "segment_sort_kernel", "cell_finish_kernel", "tile_ranges_kernel",
                                                                "scan_emit_kernel"))
    passes = launches(ran, "onesweep_pass_kernel<4, true>")
    if plan == "radix":
        assert sort == 1 and seg == 0 and cell == 0 and ranges == binnings and emit == binnings, ran
    elif plan in ("seg", "seg3"):
        assert seg == binnings and sort == 0 and cell == 0 and ranges == 0 and emit == binnings and passes == binnings * (2 if plan == "seg3" else 1), ran
    elif plan == "cells":
        assert cell == binnings and sort == 0 and seg == 0 and ranges == 0 and passes == 0 and emit == binnings, ran
    else:
        assert ranges == binnings and sort == 0 and seg == 0 and cell == 0 and passes == binnings, ran
        assert emit == (binnings if plan == "bucket" or not speculative else binnings - 1), ran


def check_slack(arena, P, cap, W, H, pattern, what):
    """The binning buffer starts with four arrays of `cap` 32-bit words (keys and values of the partition passes' ping-pong; the emission
    writes the first), each rounded up to 256 bytes: csrc/api.hip compute_layout, whose public point_list offset is the fourth's (one pass)
    or the third's.  A kernel that runs past entry `cap` of one of them — a missing clamp to the capacity — lands in the next array of the
    same buffer, where no band can see it; it crosses the rounding slack first, which nothing ever writes: the slack must still hold the
    pattern the buffer was poisoned with."""
    from das3r_amd import _lib
    from tests.guard_bands import pattern_bytes
    L = _lib.layout(P, cap, W, H)
    stride = (4 * cap + 255) // 256 * 256
    assert L["point_list"] in (2 * stride, 3 * stride) and arena.nbytes >= L["binning_bytes"], (L["point_list"], stride, arena.nbytes)
    slack = stride - 4 * cap
    assert slack > 0, f"{what}: a capacity of {cap} leaves no slack to look at"
    want = torch.tensor(list(pattern_bytes(pattern, slack)), dtype=torch.uint8)   # (4 * cap is a multiple of 4: the word pattern starts over)
    for k in range(4):
        got = arena.payload()[k * stride + 4 * cap:(k + 1) * stride].cpu()
        assert torch.equal(got, want), f"{what}: array {k} of the binning buffer ({arena!r}) was written past entry {cap}: {int((got != want).sum())} of {slack} slack bytes changed"


_SMALL = {}


def _count_at(mod, setenv):
    """num_rendered of big_splats at a scale modifier (the count an overflow's speculative capacity was laid out from)"""
    if mod not in _SMALL:
        from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
        scd = cell_scene("big_splats").to(_dev())
        e = torch.empty(0, device=_dev())
        rs = GaussianRasterizationSettings(**{**scd.settings_kwargs(), "scale_modifier": mod})
        _lib.forget_shapes()
        _SMALL[mod] = int(rasterizer._forward_full(rs, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e, exact=True)[0])
    return _SMALL[mod]


_EXACT = {}


def _cell_result(res):
    """tests/test_gpu_cell_sort.py run()'s result as a nest of tensors and numbers (the launch table apart)"""
    return {k: v for k, v in res.items() if k != "ran"}


def check_regime(regime, res, plan, setenv, guard=None):
    """What a regime must look like, so that none passes unreached; with a guard, what the registry must hold."""
    I, cap = res["I"], res["cap"]
    if regime == "exact":
        assert cap == I
    elif plan == "radix":
        assert cap == I, "the global sort never speculates: its buffer is laid out for the count it waited for"
    elif regime == "fits":
        assert cap > I, "the second forward speculates with headroom"
    else:
        small = _count_at(0.15, setenv)
        assert cap == I and I > small + small // 4 + 4096, "the scene outgrew the speculative capacity and the forward was redone exactly"
    if guard is not None:
        mine = guard.from_site(ALLOC_SITE)
        buffers = [a for a in mine if "(fn)" in a.site]   # (_Alloc's callbacks: geom, img and binning of every forward under the guard)
        forwards = 1 + len(REGIMES[regime].get("before", ()))
        redone = regime == "overflow" and plan in SPECULATING
        assert len(buffers) == 3 * forwards + (1 if redone else 0), [repr(a) for a in buffers]
        sc = cell_scene("big_splats")
        check_slack(buffers[-1], sc.P, cap, sc.W, sc.H, guard.pattern, f"{plan or 'unset'} {regime}")   # (the final buffer, whatever the regime)
        if redone:   # the last forward asked for geom, img, the speculative binning buffer and the exact one: both are in the registry
            from das3r_amd import _lib
            small = _count_at(0.15, setenv)
            spec, exact = buffers[-2], buffers[-1]
            # (the plan's capacity: the last count + 25 % + 4096; the segmented plans lay the same instances out with their bucket bits)
            assert exact.nbytes == _lib.layout(sc.P, I, sc.W, sc.H)["binning_bytes"] and spec.nbytes < exact.nbytes
            assert spec.nbytes == _lib.layout(sc.P, small + small // 4 + 4096, sc.W, sc.H)["binning_bytes"], (spec.nbytes, small)
            # (the first attempt met more instances than this buffer holds: every store past the capacity must have been dropped)
            check_slack(spec, sc.P, small + small // 4 + 4096, sc.W, sc.H, guard.pattern, f"{plan or 'unset'} {regime}, the superseded buffer")


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("plan", PLANS, ids=[p or "unset" for p in PLANS])
def test_forward_plans_and_capacity_regimes(plan, regime, monkeypatch):
    """tests/test_gpu_cell_sort.py's big_splats (P = 1200, 128 x 64) through its run(): under every plan, laid out exactly, speculatively with
    headroom, and speculatively too small — where the first attempt's kernels must clamp EVERY store to the capacity (emission, partition passes,
    cell cursors, segment sort, tile ranges, bucket checkpoints) before the forward is redone: the superseded binning buffer stays in the
    registry and its bands are checked with the others.  The results also equal a DAS3R_CAPACITY=exact run's."""
    sc = cell_scene("big_splats")
    kw = REGIMES[regime]

    def op(guard):
        res = cell_run(sc, plan, monkeypatch.setenv, profile=True, **kw)
        print(f"[{plan or 'unset'} {regime}{' guarded' if guard else ''}] num_rendered {res['I']} capacity {res['cap']} ran {res['ran']}")
        assert_plan_ran(plan, res["ran"], 2 if regime == "overflow" and plan in SPECULATING else 1, regime != "exact")
        check_regime(regime, res, plan, monkeypatch.setenv, guard)
        return _cell_result(res)

    base = four_runs(op, f"big_splats, DAS3R_BINNING={plan or 'unset'}, {regime}")
    if plan not in _EXACT:
        monkeypatch.setenv("DAS3R_CAPACITY", "exact")
        _EXACT[plan] = _cell_result(cell_run(sc, plan, monkeypatch.setenv, exact=False, before=(1.0,)))
        monkeypatch.delenv("DAS3R_CAPACITY")
        assert _EXACT[plan]["cap"] == _EXACT[plan]["I"], "DAS3R_CAPACITY=exact switches the speculation off"
    assert_same_bits(_without(base, "cap"), _without(_EXACT[plan], "cap"), f"{plan or 'unset'} {regime} vs DAS3R_CAPACITY=exact")


def _big_inputs(degree3=False):
    """tests/test_gpu_cell_sort.py's big_splats (degree 1), or the same scene with SH of degree 3"""
    from das3r_amd.synth import make_scene
    key = ("big_splats", degree3)
    if key not in _INPUTS:
        sc = cell_scene("big_splats") if not degree3 else make_scene(P=1200, W=128, H=64, focal=100.0, sh_degree=3, seed=62, s_px=(3.0, 10.0), opacity=0.05)
        _inputs(key, (sc, dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)))
    return _INPUTS[key]


def _driven(what, plan, regime, monkeypatch, inputs, **kw):
    monkeypatch.setenv("DAS3R_BINNING", plan)
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")

    def op(guard):
        res, ran = drive(None, inputs=inputs, profile=True, **REGIMES[regime], **kw)
        print(f"[{what}{' guarded' if guard else ''}] num_rendered {res['I']} capacity {res['cap']} ran {ran}")
        assert_plan_ran(plan, ran, 2 if regime == "overflow" else 1, regime != "exact")
        assert res["cap"] == res["I"] if regime != "fits" else res["cap"] > res["I"], (regime, res["I"], res["cap"])
        if guard is not None:
            buffers = [a for a in guard.from_site(ALLOC_SITE) if "(fn)" in a.site]
            assert len(buffers) == 3 * (1 + len(REGIMES[regime].get("before", ()))) + (regime == "overflow"), [repr(a) for a in buffers]
        return res

    return four_runs(op, what)


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("plan", ["", "local", "cells"], ids=["unset", "local", "cells"])
@pytest.mark.parametrize("form", ["invdepth", "antialiasing"])
def test_forward_plans_with_an_inverse_depth_image_and_antialiased(form, plan, regime, monkeypatch):
    """The same scene and regimes with an inverse-depth image (the binning buffer is asked for with d_bytes, not binning_bytes: the depth
    checkpoints lie behind the lists) and with the antialiasing factor; the backward is the inverse-depth one where there is an image."""
    res = _driven(f"big_splats {form}, DAS3R_BINNING={plan or 'unset'}, {regime}", plan, regime, monkeypatch, _big_inputs(), **{form: True})
    assert ("invdepth" in res) == (form == "invdepth") and len(res["grads"]) == 1


@pytest.mark.parametrize("regime", list(REGIMES))
def test_forward_at_sh_degree_3(regime, monkeypatch):
    """Degree 3: the geometry buffer is geom_bytes plus the nine SH-Jacobian planes, which the per-Gaussian backward reads."""
    res = _driven(f"big_splats at degree 3, unset, {regime}", "", regime, monkeypatch, _big_inputs(degree3=True))
    assert res["grads"][0]["shs"].shape == (1200, 16, 3)


def _all_culled():
    sc, mode = util.scene_variant("culled")
    from das3r_amd.synth import Scene
    means = sc.means3D.clone()
    means[:, 2] = -means[:, 2].abs() - 0.5   # every splat behind the camera
    return Scene(**{**sc.__dict__, "means3D": means.contiguous()}), mode


@pytest.mark.parametrize("case", ["fused_emit_off", "single", "all_culled", "no_gaussians"])
def test_forward_without_fused_emission_and_on_degenerate_scenes(case, monkeypatch):
    """DAS3R_FUSED_EMIT=0 (a speculative second forward through scan_emit_kernel instead of the emission inside the preprocess kernel); one
    Gaussian; a scene whose every Gaussian is culled (num_rendered 0: a binning buffer for no instance); no Gaussian at all."""
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    if case == "no_gaussians":
        from das3r_amd import GaussianRasterizationSettings, rasterizer
        sc, skw, _args, _dL, _dD = _inputs("single")
        e = torch.empty(0, 3, device=_dev())

        def op(guard):
            out = rasterizer._forward_full(GaussianRasterizationSettings(**skw), e, torch.empty(0, 16, 3, device=_dev()), e[:, :0], e[:, :1], e, e[:, :0], e[:, :0],
                                           invdepth=True)
            assert out[0] == 0 and not out[1].any() and not out[7].any() and out[2].numel() == 0
            return dict(color=out[1].cpu(), invdepth=out[7].cpu())

        four_runs(op, "P = 0")
        return
    if case == "fused_emit_off":
        monkeypatch.setenv("DAS3R_FUSED_EMIT", "0")
    name = {"fused_emit_off": "basic_deg3", "single": "single", "all_culled": "all_culled"}[case]
    if case == "all_culled":
        _inputs(name, _all_culled())
    for regime, kw in REGIMES.items():
        if regime == "overflow":
            continue   # (these scenes do not outgrow a capacity: that regime is the plans' test above)

        def op(guard):
            res, ran = drive(name, profile=True, **kw)
            print(f"[{case} {regime}{' guarded' if guard else ''}] num_rendered {res['I']} capacity {res['cap']} ran {ran}")
            if case == "fused_emit_off" and regime == "fits":
                assert res["cap"] > res["I"] and launches(ran, "scan_emit_kernel") == 1, ran
            if case == "all_culled":
                assert res["I"] == 0 and not res["radii"].any()
            if case == "single":
                assert res["I"] > 0 and res["radii"].numel() == 1
            return res

        four_runs(op, f"{case}, {regime}")


# ------------------------------------------------------------------------------------------------------------------- forward kernels
FWD_KERNELS = {"quad": "render_forward_kernel", "rows": "render_forward_rows_kernel", "lanes": "render_forward_lanes_kernel",
               "slices": "render_forward_slices", "fine": "render_forward_regions_kernel"}   # tests/test_gpu_aux.py's KERNELS, and the slices
FWD_BINNING = {"quad": "radix", "rows": "local", "lanes": "radix", "slices": "radix", "fine": "radix"}   # (its PATHS: lists in the local order take the rows kernel whatever is forced)


@pytest.mark.parametrize("name", ["ragged_image", "long_lists"])
@pytest.mark.parametrize("kernel", list(FWD_KERNELS))
def test_forward_kernels(kernel, name, monkeypatch):
    """Every compositing forward kernel forced, on an image whose last tiles are partial and on lists of several batches."""
    monkeypatch.setenv("DAS3R_RENDER", kernel)
    monkeypatch.setenv("DAS3R_BINNING", FWD_BINNING[kernel])
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")

    def op(guard):
        res, ran = drive(name, profile=True)
        print(f"[{name} DAS3R_RENDER={kernel}] {ran}")
        assert launches(ran, FWD_KERNELS[kernel]) >= 1, ran
        assert [k for k in ran if k.startswith("render_forward") and not k.startswith(FWD_KERNELS[kernel])] == [], ran
        return res

    four_runs(op, f"{name}, DAS3R_RENDER={kernel}")


# --------------------------------------------------------------------------------------------------------- backward scratch and gradients
MISALIGNS = (0, 4, 8, 12)
BWD_KINDS = {   # DAS3R_RENDER_BWD (None: unset) -> (the rest of the environment, the kernel that must have run)
    "unset": ({}, "render_backward"), "dpp": ({}, "render_backward_kernel"), "blk64": ({}, "render_backward_blk_kernel<64"),
    "blk128p1": ({}, "render_backward_blk_kernel<128, 1"), "blk192": ({}, "render_backward_blk_kernel<192"),
    "blk256": ({}, "render_backward_blk_kernel<256"), "fine128": ({"DAS3R_RENDER": "fine"}, "render_backward_regions_kernel<128"),
    "blk128+buckets4": ({"DAS3R_BWD_BUCKETS": "4"}, "render_backward_blk_kernel<128"),
    "fine128+buckets4": ({"DAS3R_RENDER": "fine", "DAS3R_BWD_BUCKETS": "4"}, "render_backward_regions_kernel<128"),
}
BWD_SCENES = ["ragged_image", "culled", "long_lists", "deep"]


def _grads_close(got, want, what):
    """The pixel-per-lane backward (DAS3R_RENDER_BWD=dpp) meets its four waves with LDS float atomics whose order varies: documented as not
    bit-reproducible run to run (csrc/kernel_choice.h Switches::deterministic, tests/test_gpu_raster.py
    test_deterministic_switch_gives_bit_identical_gradients).  Its gradients are held to the project's bar between two backward kernels
    (util.assert_grad_close, tests/test_gpu_raster.py test_backward_kernels_agree); everything else of the run to the same bits."""
    assert_same_bits(_without(got, "grads"), _without(want, "grads"), what)
    for a, b in zip(got["grads"], want["grads"]):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.isfinite(a[k]).all(), f"{what}: dL/d{k}"
            util.assert_grad_close(a[k].numpy(), b[k].numpy(), f"{what}: dL/d{k}", tol=5e-5)


@pytest.mark.parametrize("name", BWD_SCENES)
@pytest.mark.parametrize("kind", list(BWD_KINDS))
def test_backward_kernels_and_scratch_alignments(kind, name, monkeypatch):
    """das3r_raster_backward under every compositing backward kernel, its scratch (das3r_raster_backward_scratch_bytes) 16-byte aligned and 4,
    8 and 12 bytes off: the per-Gaussian backward reads a workgroup's run of partial rows as 16-byte words when it can — no such load or
    store may cover a tail shorter than 16 bytes.  One forward, four backwards per run."""
    env, kernel = BWD_KINDS[kind]
    if kind != "unset":
        monkeypatch.setenv("DAS3R_RENDER_BWD", kind.split("+")[0])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if kind != "dpp":
        monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")

    def op(guard):
        res, ran = drive(name, misaligns=MISALIGNS, profile=True)
        assert launches(ran, kernel) == len(MISALIGNS), ran
        if guard is not None:
            scratch = [a for a in guard.from_site(ALLOC_SITE) if "(_scratch)" in a.site]
            assert len(scratch) == len(MISALIGNS) and [a.nbytes - scratch[0].nbytes for a in scratch] == list(MISALIGNS)
        if kind != "dpp":
            for g in res["grads"][1:]:
                assert_same_bits(g, res["grads"][0], f"{name} [{kind}]: a misaligned scratch")
        return res

    four_runs(op, f"{name}, DAS3R_RENDER_BWD={kind}", compare=_grads_close if kind == "dpp" else assert_same_bits)


@pytest.mark.parametrize("name", BWD_SCENES + ["cov3D_precomp", "colors_precomp"])
@pytest.mark.parametrize("form", ["colour", "depth", "focal", "focal+depth"])
def test_backward_forms_and_precomputed_inputs(form, name, monkeypatch):
    """das3r_raster_backward_depth (das3r_raster_backward_depth_scratch_bytes) and das3r_raster_backward_focal with per-splat rows
    (das3r_raster_focal_workspace_bytes), on the same scenes and alignments, and all forms on cov3D_precomp / colors_precomp inputs (the
    gradient set then has dL/dcov3D / dL/dcolors instead of scales + rotations / SH)."""
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    depth, focal = "depth" in form, "focal" in form

    def op(guard):
        res, _ = drive(name, misaligns=MISALIGNS, invdepth=depth, focal=focal)
        for g in res["grads"][1:]:
            assert_same_bits(g, res["grads"][0], f"{name} [{form}]: a misaligned scratch")
        g = res["grads"][0]
        assert ("cov" in g) == (name == "cov3D_precomp") and ("colors" in g) == (name == "colors_precomp") and ("focal_per_splat" in g) == focal
        if guard is not None and focal:
            assert len([a for a in guard.from_site(ALLOC_SITE) if "(_backward)" in a.site and a.name == "torch.empty"]) >= len(MISALIGNS), "the workspace"
        return res

    four_runs(op, f"{name}, {form} backward")


# ------------------------------------------------------------------------------------------------------------------- saved-list calls
def _state_of(name, **more):
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    sc, skw, args, _dL, _dD = _inputs(name)
    rs = GaussianRasterizationSettings(**skw)
    _lib.forget_shapes()
    res = rasterizer._forward_full(rs, *args, **more)
    return sc, rs, args, rasterizer.RasterState.of(res, rs)


def _rand(*shape, seed=77):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(_dev())


@pytest.mark.parametrize("name", ["single", "culled", "long_lists"])
@pytest.mark.parametrize("C_", [1, 8, 9], ids=["C1", "C8", "C9"])
def test_aux_channels_and_coverage(C_, name, monkeypatch):
    """composite_features, feature_adjoint (das3r_raster_aux_scratch_bytes) and the coverage image with 1, DAS3R_AUX_MAX_CHANNELS and one
    channel more (two library calls), then the aux / coverage backward to the geometry (das3r_raster_aux_backward_scratch_bytes) through
    autograd, forward included: the saved buffers the calls read are poisoned too."""
    from das3r_amd import _lib, rasterizer
    from das3r_amd.rasterizer import AuxGeometry, alpha_of, composite_features, feature_adjoint
    assert _lib.AUX_MAX_CHANNELS == 8
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    sc = _inputs(name)[0]
    F, G, Ga = _rand(sc.P, C_).abs(), _rand(C_, sc.H, sc.W, seed=78) / (sc.H * sc.W), _rand(1, sc.H, sc.W, seed=79) / (sc.H * sc.W)

    def op(guard):
        _sc, rs, args, state = _state_of(name)
        image = composite_features(state, F)
        adjoint = feature_adjoint(state, G)
        added = feature_adjoint(state, G, out=torch.ones(sc.P, C_, device=_dev()), accumulate=True)
        alpha = alpha_of(state)
        means3D, _shs, _cols, opacities, scales, rotations, _cov = args
        leaves = [t.clone().requires_grad_(True) for t in (F, means3D, opacities, scales, rotations)]
        means2D = torch.zeros(sc.P, 3, device=_dev(), requires_grad=True)
        geometry = AuxGeometry(rs, leaves[1], means2D, leaves[2], shs=args[1], scales=leaves[3], rotations=leaves[4])
        img2 = composite_features(state, leaves[0], geometry=geometry)
        cov = alpha_of(state, geometry=geometry)
        ((img2 * G).sum() + (cov * Ga).sum()).backward()
        # the raw call too, its scratch 4, 8 and 12 bytes off
        n = min(C_, 8)
        raw = [rasterizer._aux_backward_impl(state, rs, F[:, :n].contiguous(), G[:n].contiguous(), Ga, True, *args, _scratch_misalign=off) for off in MISALIGNS]
        torch.cuda.synchronize()
        for r in raw[1:]:
            assert_same_bits(r, raw[0], f"{name} C = {C_}: a misaligned aux-backward scratch")
        return dict(image=image, adjoint=adjoint, added=added, alpha=alpha, image2=img2.detach(), coverage=cov.detach(),
                    grads=[t.grad for t in leaves + [means2D]], raw=raw[0])

    four_runs(op, f"{name}, aux channels C = {C_}")


@pytest.mark.parametrize("name", ["single", "culled", "deep"])
def test_distortion_and_median(name, monkeypatch):
    """The ray-distortion regulariser forward and backward (das3r_raster_distortion_backward_scratch_bytes, every alignment) and the median
    depth with both hit planes and median_hit_adjoint (das3r_raster_median_scratch_bytes)."""
    from das3r_amd import rasterizer
    from das3r_amd.rasterizer import median_depth_of, median_hit_adjoint
    monkeypatch.setenv("DAS3R_DETERMINISTIC", "1")
    sc = _inputs(name)[0]
    G = _rand(1, sc.H, sc.W, seed=81) / (sc.H * sc.W)

    def op(guard):
        _sc, rs, args, state = _state_of(name)
        D, totals = rasterizer._distortion_forward(state, True)
        back = [rasterizer._distortion_backward_impl(state, rs, G, totals, *args, _scratch_misalign=off) for off in MISALIGNS]
        out = dict(D=D, totals=totals, plain=rasterizer.distortion_of(state), back=back[0])
        for tau in (0.5, 0.05):
            depth, hit_g, hit_p = median_depth_of(state, threshold=tau, return_hit=True, return_position=True)
            dz = median_hit_adjoint(state, G, hit_p)
            added = median_hit_adjoint(state, G, hit_p, out=torch.ones(sc.P, device=_dev()), accumulate=True)
            out[f"median{tau}"] = (depth, hit_g, hit_p, dz, added)
        torch.cuda.synchronize()
        for b in back[1:]:
            assert_same_bits(b, back[0], f"{name}: a misaligned distortion scratch")
        return out

    four_runs(op, f"{name}, distortion and median depth")


@pytest.mark.parametrize("P", [1, 63, 65, 257])
def test_gaussian_normals(P):
    """Per-Gaussian normals forward (normals and the uint8 choice plane: P bytes, the only buffer here that is no multiple of 4) and backward,
    through autograd."""
    from das3r_amd import gaussian_normals
    from tests.test_gpu_normals import CAMPOS, _rows, _settings, _view as view_matrix
    q, s, mu, _ = (t.to(_dev()) for t in _rows(P))
    rs = _settings(view_matrix(), CAMPOS)
    G = _rand(P, 3, seed=5)

    def op(guard):
        leaf = q.clone().requires_grad_(True)
        normals = gaussian_normals(rs, leaf, s, mu)
        (normals * G).sum().backward()
        with torch.no_grad():
            plain = gaussian_normals(rs, q, s, mu)
        return dict(normals=normals.detach(), plain=plain, g_rotations=leaf.grad)

    four_runs(op, f"gaussian normals, P = {P}")


@pytest.mark.parametrize("shape", [(1, 5), (3, 3), (17, 19), (33, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_normal_consistency(shape):
    """depth_normals and the normal-consistency loss image forward and backward on the image kernels' edge shapes (their tile is 32 x 8)."""
    from das3r_amd import depth_normals, normal_consistency
    from tests.test_gpu_normals import TANFOV, _image_case, _settings
    H, W = shape
    z, normal, alpha, mask, G = (t.to(_dev()) for t in _image_case(H, W, 7))
    rs = _settings(torch.eye(4), (0.0, 0.0, 0.0), H, W, TANFOV)

    def op(guard):
        leaves = [t.clone().requires_grad_(True) for t in (z, normal, alpha)]
        loss = normal_consistency(*leaves, rs, mask=mask)
        (loss * G).sum().backward()
        return dict(N=depth_normals(z, rs), loss=loss.detach(), unmasked=normal_consistency(z, normal, alpha, rs), grads=[t.grad for t in leaves])

    four_runs(op, f"normal consistency, {H} x {W}")
