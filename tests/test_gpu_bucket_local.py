"""The fourth binning plan — segmented emission, local finish (csrc/path_policy.h bucket_local_rule, DAS3R_BINNING=bucket): the instances
are emitted and partitioned with a depth bucket and sixteen fraction bits in the key, no segment_sort_kernel runs, and the compositing
kernel finishes a list of 257 - 512 entries by ranking every entry inside its (tile, bucket) segment on the key words (render_common.h
local_order_tile); entries that tie on bucket and fraction are ranked again on their depth bits; every other list length takes the local
order's branches.

Small images with the plan forced (32 tiles of 16 x 16 pixels: five bits of tile id, one partition pass, three bucket bits), a few
thousand small splats so that the tile lists land in 257 - 512: the smallest shapes at which each branch is reached.  Lists, ranges,
num_rendered, image, final_T, n_contrib and the gradients must be THE SAME BITS as the global sort's (DAS3R_BINNING=radix) and the forced
local order's, the lists the oracle's, and image and gradients within the parity bars of the oracle.  The references are computed once per
scene and shared."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

MODE = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
W, H = 128, 64
TILES = (W // 16) * (H // 16)
GRADS = ("means2D", "colors", "opacities", "means3D", "cov", "shs", "scales", "rotations")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _view(buf, off, dtype, count):
    item = torch.tensor([], dtype=dtype).element_size()
    return buf[off:off + count * item].view(dtype)


def _at_depths(sc, z_new):
    """The scene with every splat moved along its ray to depth z_new: same pixel (up to rounding), same footprint in pixels."""
    from das3r_amd.synth import Scene
    f = (z_new / sc.means3D[:, 2]).to(torch.float32)
    means = sc.means3D * f[:, None]
    means[:, 2] = z_new   # (the view matrix is the identity: exactly these depth bits, not z * f rounded)
    return Scene(**{**sc.__dict__, "means3D": means.contiguous(), "scales": (sc.scales * f[:, None]).contiguous()})


def _scene(case):
    from das3r_amd.synth import make_scene
    g = torch.Generator().manual_seed(77)
    if case == "density_gradient":   # crowded towards the top: lists of <= 256, 257 - 512 and 513 - 1024 entries in one image; empty tiles: below
        sc = make_scene(P=8200, W=W, H=H, focal=100.0, sh_degree=1, seed=63, s_px=(0.5, 2.0), opacity=0.05, y_skew=3.0)
        keep = sc.means3D[:, 0] / sc.means3D[:, 2] * 100.0 + W / 2 < W - 32.0      # nothing reaches the last column of tiles
        from das3r_amd.synth import Scene
        per = {k: (v[keep].contiguous() if torch.is_tensor(v) and v.shape[:1] == (sc.P,) else v) for k, v in sc.__dict__.items()}
        return Scene(**per)
    if case == "big_splats":   # footprints of several tiles that shrink to one at scale modifier 0.15: the scene outgrows a speculative capacity
        return make_scene(P=1200, W=W, H=H, focal=100.0, sh_degree=1, seed=62, s_px=(3.0, 10.0), opacity=0.05)
    sc = make_scene(P=5600, W=W, H=H, focal=100.0, sh_degree=1, seed=61, s_px=(0.5, 2.0), opacity=0.05)
    if case == "random":
        return sc
    if case == "one_depth":
        return _at_depths(sc, torch.full((sc.P,), 4.0))
    if case == "two_depths":
        return _at_depths(sc, torch.tensor([3.0, 5.5])[torch.randint(0, 2, (sc.P,), generator=g)])
    raise KeyError(case)


def run(sc, binning, setenv, invdepth=False, before=(), exact=True, profile=False):
    """One forward + backward through the C entry with DAS3R_BINNING=binning -> everything a forward leaves behind, on the host."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    dev = _dev()
    setenv("DAS3R_BINNING", binning)
    setenv("DAS3R_RECT", "upstream")   # (bin over upstream's square: the oracle's lists)
    scd = sc.to(dev)
    e = torch.empty(0, device=dev)

    def forward(mod):
        rs = GaussianRasterizationSettings(**{**scd.settings_kwargs(), "scale_modifier": mod})
        return rs, rasterizer._forward_full(rs, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e, exact=exact, invdepth=invdepth)

    _lib.forget_shapes()
    for mod in before:
        forward(mod)
    torch.cuda.synchronize()
    _lib.profile_report()
    _lib.profile_enable(profile)
    try:
        rs, out = forward(1.0)
        I, color, radii, geom, binning_buf, img, cap = out[:7]
        grad_inv = torch.full((1, sc.H, sc.W), 1.0 / (sc.W * sc.H), device=dev) if invdepth else None
        grads = rasterizer._backward_impl(rs, I, scd.dL_dpix, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e, geom, binning_buf, img, cap,
                                          grad_invdepth=grad_inv)
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    ran = {k: n for k, (n, _ms) in _lib.profile_report(raw=True).items()} if profile else None
    L = _lib.layout(sc.P, int(cap), sc.W, sc.H)
    npix = sc.W * sc.H
    res = dict(I=int(I), cap=int(cap), color=color.cpu(), radii=radii.cpu(),
               point_list=_view(binning_buf, L["point_list"], torch.int32, int(I)).cpu().numpy().astype(np.uint32),
               ranges=_view(img, L["ranges"], torch.int32, 2 * TILES).cpu().numpy().reshape(TILES, 2).astype(np.uint32),
               final_T=_view(img, L["final_T"], torch.int32, npix).cpu(), n_contrib=_view(img, L["n_contrib"], torch.int32, npix).cpu(),
               grads={k: t.cpu() for k, t in zip(GRADS, grads) if t is not None and t.numel()}, ran=ran)
    if invdepth:
        res["invdepth"] = out[7].cpu()
    return res


_REFS = {}


def refs(case, setenv, invdepth=False):
    """The global sort's and the forced local order's results of a scene, and the oracle's: computed once."""
    key = (case, invdepth)
    if key not in _REFS:
        sc = _scene(case)
        _REFS[key] = (sc, run(sc, "radix", setenv, invdepth), run(sc, "local", setenv, invdepth), util.run_oracle(sc, MODE))
    return _REFS[key]


def lengths(r):
    return (r["ranges"][:, 1] - r["ranges"][:, 0]).astype(np.int64)


def assert_same_bits(got, want, what):
    assert got["I"] == want["I"], what
    for k in ("ranges", "point_list"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k}"
    for k in ("color", "radii", "final_T", "n_contrib") + (("invdepth",) if "invdepth" in want else ()):
        assert torch.equal(got[k], want[k]), f"{what}: {k}"
    assert got["grads"].keys() == want["grads"].keys()
    for k, t in got["grads"].items():
        same = torch.equal(t, want["grads"][k])
        print(f"{what}: dL/d{k} {'same bits' if same else 'max |delta| %.3g' % float((t - want['grads'][k]).abs().max())}")
        assert same, f"{what}: dL/d{k}"


def assert_oracle(got, oracle, what, grads=True):
    ref_color, ref_radii, ref_g, S = oracle
    assert got["I"] == S["num_rendered"]
    assert np.array_equal(got["ranges"], S["ranges"]) and np.array_equal(got["point_list"], S["point_list"]), f"{what}: the oracle's lists"
    assert np.array_equal(got["radii"].numpy(), ref_radii)
    util.assert_color_close(got["color"].numpy(), ref_color, what)
    for k in () if not grads else ("means3D", "opacities", "shs", "scales", "rotations", "means2D"):
        util.assert_grad_close(got["grads"][k].numpy(), ref_g[k], f"{what} dL/d{k}")
        util.assert_grad_elementwise(got["grads"][k].numpy(), ref_g[k], f"{what} dL/d{k}")


def check_case(case, setenv, invdepth=False, **kw):
    sc, radix, local, oracle = refs(case, setenv, invdepth)
    got = run(sc, "bucket", setenv, invdepth, **kw)
    n = lengths(got)
    print(f"{case}: num_rendered {got['I']}, lists min {n.min()} mean {n.mean():.0f} max {n.max()}, "
          f"{int(((n > 256) & (n <= 512)).sum())} of {TILES} in 257 - 512")
    # (the gradients too: every backward kernel these shapes take adds a pixel's and a Gaussian's terms in list order)
    assert_same_bits(got, local, f"{case}: bucket vs local")
    assert_same_bits(got, radix, f"{case}: bucket vs radix")
    assert_oracle(got, oracle, case, grads=not invdepth)   # (the oracle's backward knows no inverse-depth image: its gradients are the colour's alone)
    return got, n


def test_random_depths(monkeypatch):
    """(a) random depths: most tiles rank their segments on the fraction bits alone, a few hold a tie group."""
    got, n = check_case("random", monkeypatch.setenv)
    assert ((n > 256) & (n <= 512)).sum() >= TILES // 2, "the scene must put its lists into the 257 - 512 branch"


@pytest.mark.parametrize("case", ["one_depth", "two_depths"])
def test_every_tile_ties(case, monkeypatch):
    """(b) all depths equal / two depth values: every segment is one tie group, resolved on (depth bits, position): the index order."""
    got, n = check_case(case, monkeypatch.setenv)
    assert ((n > 256) & (n <= 512)).sum() >= TILES // 2
    for a, b in got["ranges"]:
        pl = got["point_list"][a:b].astype(np.int64)
        if case == "one_depth":
            assert (np.diff(pl) > 0).all(), "one depth: a tile's list is in index order"


def test_every_branch_in_one_image(monkeypatch):
    """(c) a density gradient: lists of <= 256, 257 - 512 and 513 - 1024 entries and empty tiles in one image."""
    got, n = check_case("density_gradient", monkeypatch.setenv)
    assert (n == 0).any() and ((n > 0) & (n <= 256)).any() and ((n > 256) & (n <= 512)).any() and ((n > 512) & (n <= 1024)).any(), sorted(n)


def test_second_forward_and_overflow_redo(monkeypatch):
    """(d) a second forward of the shape (speculative capacity: laid out with headroom, the kernels clamp), and a forward whose scene has
    outgrown the speculative capacity (scale modifier 0.15, then 1.0): binning and compositing are redone at the exact size."""
    sc, radix, local, oracle = refs("random", monkeypatch.setenv)
    second = run(sc, "bucket", monkeypatch.setenv, before=(1.0,), exact=False)
    assert second["cap"] > second["I"], "the second forward speculates with headroom"
    assert_same_bits(second, local, "second forward vs local")
    sc, radix, local, oracle = refs("big_splats", monkeypatch.setenv)
    redo = run(sc, "bucket", monkeypatch.setenv, before=(0.15,), exact=False)
    n = lengths(redo)
    print(f"big_splats: num_rendered {redo['I']}, lists min {n.min()} mean {n.mean():.0f} max {n.max()}")
    assert redo["cap"] == redo["I"], "the redone forward is laid out exactly"
    assert ((n > 256) & (n <= 512)).sum() >= TILES // 2
    assert_same_bits(redo, local, "overflow redo vs local")
    assert_same_bits(redo, radix, "overflow redo vs radix")


# recorded once from this branch on an MI355X, after test_random_depths passed: one forward (second of its shape) + backward
LAUNCHES = {   # num_rendered 11801, capacity 18847
    "onesweep_pass_kernel<4, true>": 1,
    "preprocess_backward_kernel<true, false, false, true, false, false, false, false, false>": 1,
    "preprocess_kernel<true, false, false>": 1,
    "render_backward_blk_kernel<128, 1, 0, 5, false>": 1,
    "render_forward_rows_kernel<false>": 1,
    "scan_emit_kernel<true, 1>": 1,
    "tile_ranges_kernel": 1,
}


def test_launch_table(monkeypatch):
    """(e) what one forward + backward under the plan launches: no segment_sort_kernel, exactly one tile_ranges_kernel."""
    sc, *_ = refs("random", monkeypatch.setenv)
    got = run(sc, "bucket", monkeypatch.setenv, before=(1.0,), exact=False, profile=True)
    print(got["ran"])
    assert not any(k.startswith("segment_sort_kernel") for k in got["ran"])
    assert got["ran"].get("tile_ranges_kernel") == 1
    assert got["ran"] == LAUNCHES


def test_inverse_depth_output(monkeypatch):
    """(f) the DEPTH instantiations: the same equalities, the inverse-depth image and its gradients included."""
    check_case("random", monkeypatch.setenv, invdepth=True)
