"""The fifth binning plan — "cells" (csrc/path_policy.h cells_rule, csrc/cell_sort.hip, DAS3R_BINNING=cells): the bucket plan's emission
and key, partitioned by the top eight partition bits into ranges reserved on per-bin cursors (cell_partition_kernel) and ordered per
cell by the low eight through LDS (cell_finish_kernel, which also writes the tile ranges).  Neither kernel is stable; the compositing
kernel ranks ties by Gaussian id (render_common.h local_order_tile), so everything a forward leaves behind must be THE SAME BITS as
under the stable plans: forced cells against forced bucket and radix, on lists, ranges, image, final_T, n_contrib, and on the gradients
under DAS3R_DETERMINISTIC=1.

Shapes: the smallest at which each path of the two kernels is reached.  Up to 64 tiles the partition key has eight bits: one cell, the
finish alone runs (24 and 33 tiles).  From 257 tiles on it has sixteen: 1040 tiles are 130 cells of eight tiles, 2064 tiles 129 cells of
sixteen.  A part of a cell (a quarter of its 256 bins) that holds more than one LDS round of 3072 entries takes several rounds: sixteen
tiles of 1250 entries in one cell (one pass), four neighbouring tiles of 850 in one part (two passes).  Lists of exactly 0, 1, 256, 257,
512 and 513 entries sit on both sides of every branch of local_order_tile; depths quantised to a few values put equal depths with
different ids into every (tile, bucket) segment.  The references are computed once per scene and shared."""
import numpy as np
import pytest
import torch

from tests.test_gpu_bucket_local import GRADS, _dev, _view, assert_same_bits
from tests.tile_grid_scenes import placed_scene   # (splats on the centres of chosen tiles; every image here is at least as wide as high: focal W / 1.28)

pytestmark = pytest.mark.gpu


LENGTHS = (1, 256, 257, 512, 513)


def _scene(case):
    from das3r_amd.synth import make_scene
    if case == "tiles24":      # fewer than 32 tiles: one partial cell
        return make_scene(P=3000, W=128, H=48, focal=100.0, sh_degree=1, seed=71, s_px=(0.5, 2.0), opacity=0.05)
    if case == "tiles33":      # 33 tiles
        return make_scene(P=4000, W=176, H=48, focal=100.0, sh_degree=1, seed=72, s_px=(0.5, 2.0), opacity=0.05)
    if case == "sparse1040":   # 1040 tiles, a few thousand splats: mostly empty tiles, some empty cells
        sc = make_scene(P=3000, W=640, H=416, focal=300.0, sh_degree=1, seed=73, s_px=(0.5, 3.0), opacity=0.2)
        from das3r_amd.synth import Scene
        keep = sc.means3D[:, 1] < 0.0   # nothing in the lower half: whole cells stay empty
        return Scene(**{k: (v[keep].contiguous() if torch.is_tensor(v) and v.shape[:1] == (sc.P,) else v) for k, v in sc.__dict__.items()})
    if case == "lengths32":    # one pass: lists of exactly 0, 1, 256, 257, 512, 513 entries, depths tied
        return placed_scene(128, 64, {3 + 5 * i: n for i, n in enumerate(LENGTHS)}, seed=74, zlevels=7)
    if case == "lengths1040":  # two passes: the same lists, in five cells
        return placed_scene(640, 416, {t: n for t, n in zip((5, 100, 333, 600, 1039), LENGTHS)}, seed=75, zlevels=7)
    if case == "rounds16":     # one cell of sixteen tiles, 20 000 instances: every part takes two rounds
        return placed_scene(64, 64, {t: 1250 for t in range(16)}, seed=76)
    if case == "rounds2064":   # two passes, sixteen tiles a cell: tiles 32 .. 35 are one part of cell 2, 3400 entries
        return placed_scene(2064, 256, {**{t: 850 for t in range(32, 36)}, 40: 300, 2063: 20}, seed=77, zlevels=9)
    if case == "big_splats":   # footprints of several tiles that shrink to one at scale modifier 0.15: the scene outgrows a speculative capacity
        return make_scene(P=1200, W=128, H=64, focal=100.0, sh_degree=1, seed=62, s_px=(3.0, 10.0), opacity=0.05)
    raise KeyError(case)


def run(sc, binning, setenv, before=(), exact=True, profile=False):
    """One forward + backward through the C entry with DAS3R_BINNING=binning -> everything a forward leaves behind, on the host."""
    from das3r_amd import GaussianRasterizationSettings, _lib, rasterizer
    dev = _dev()
    setenv("DAS3R_BINNING", binning)
    setenv("DAS3R_DETERMINISTIC", "1")
    scd = sc.to(dev)
    e = torch.empty(0, device=dev)
    tiles = ((sc.W + 15) // 16) * ((sc.H + 15) // 16)

    def forward(mod):
        rs = GaussianRasterizationSettings(**{**scd.settings_kwargs(), "scale_modifier": mod})
        return rs, rasterizer._forward_full(rs, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e, exact=exact, invdepth=False)

    _lib.forget_shapes()
    for mod in before:
        forward(mod)
    torch.cuda.synchronize()
    _lib.profile_report()
    _lib.profile_enable(profile)
    try:
        rs, out = forward(1.0)
        I, color, radii, geom, binning_buf, img, cap = out[:7]
        grads = rasterizer._backward_impl(rs, I, scd.dL_dpix, scd.means3D, scd.shs, e, scd.opacities, scd.scales, scd.rotations, e, geom, binning_buf, img, cap,
                                          grad_invdepth=None)
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(False)
    ran = {k: n for k, (n, _ms) in _lib.profile_report(raw=True).items()} if profile else None
    L = _lib.layout(sc.P, int(cap), sc.W, sc.H)
    npix = sc.W * sc.H
    res = dict(I=int(I), cap=int(cap), color=color.cpu(), radii=radii.cpu(),
               point_list=_view(binning_buf, L["point_list"], torch.int32, int(I)).cpu().numpy().astype(np.uint32),
               ranges=_view(img, L["ranges"], torch.int32, 2 * tiles).cpu().numpy().reshape(tiles, 2).astype(np.uint32),
               final_T=_view(img, L["final_T"], torch.int32, npix).cpu(), n_contrib=_view(img, L["n_contrib"], torch.int32, npix).cpu(),
               grads={k: t.cpu() for k, t in zip(GRADS, grads) if t is not None and t.numel()}, ran=ran)
    return res


_REFS = {}


def refs(case, setenv):
    """The scene and its results under the forced bucket plan and the global sort: computed once."""
    if case not in _REFS:
        sc = _scene(case)
        _REFS[case] = (sc, run(sc, "bucket", setenv), run(sc, "radix", setenv))
    return _REFS[case]


def lengths(r):
    return (r["ranges"][:, 1] - r["ranges"][:, 0]).astype(np.int64)


def check_case(case, setenv, radix_image=True, **kw):
    sc, bucket, radix = refs(case, setenv)
    got = run(sc, "cells", setenv, profile=True, **kw)
    n = lengths(got)
    print(f"{case}: num_rendered {got['I']}, {len(n)} tiles, lists min {n.min()} mean {n.mean():.0f} max {n.max()}, {int((n == 0).sum())} empty; ran {got['ran']}")
    assert any(k.startswith("cell_finish_kernel") for k in got["ran"]), "the plan under test ran"
    assert not any(k.startswith(("onesweep_pass_kernel", "tile_ranges_kernel", "segment_sort_kernel")) for k in got["ran"])
    assert_same_bits(got, bucket, f"{case}: cells vs bucket")
    if radix_image:
        assert_same_bits(got, radix, f"{case}: cells vs radix")
    else:   # (lists beyond LOCAL_MAX: the global sort's lists are composited by another kernel than the local order's, also under the bucket plan)
        assert got["I"] == radix["I"] and np.array_equal(got["ranges"], radix["ranges"]) and np.array_equal(got["point_list"], radix["point_list"])
    return got, n


@pytest.mark.parametrize("case", ["tiles24", "tiles33"])
def test_one_cell(case, monkeypatch):
    """Fewer than 32 tiles and 33 tiles: eight partition bits, the finish alone, on the emitted triples."""
    got, n = check_case(case, monkeypatch.setenv)
    assert len(n) == {"tiles24": 24, "tiles33": 33}[case]
    assert not any(k.startswith("cell_partition_kernel") for k in got["ran"])


def test_mostly_empty_tiles_and_cells(monkeypatch):
    """1040 tiles and a few thousand splats: two passes' worth of key, most tiles empty, the lower half's cells empty."""
    got, n = check_case("sparse1040", monkeypatch.setenv)
    assert len(n) == 1040 and (n == 0).sum() > 440 and (n[600:] == 0).all() and got["I"] > 1000   # (cells 75 .. 129: tiles 600 .. 1039)
    assert any(k.startswith("cell_partition_kernel") for k in got["ran"])
    assert (got["ranges"][n == 0] == 0).all(), "an empty tile keeps the zeroes the preprocess kernel left"


@pytest.mark.parametrize("case", ["lengths32", "lengths1040"])
def test_exact_list_lengths_with_tied_depths(case, monkeypatch):
    """Lists of exactly 0, 1, 256, 257, 512 and 513 entries, every (tile, bucket) segment full of equal depths with different ids."""
    got, n = check_case(case, monkeypatch.setenv)
    assert sorted(set(n.tolist())) == [0, *LENGTHS]
    for a, b in got["ranges"]:   # equal depths come out in id order: the tie rule, whatever the arrival order
        pl = got["point_list"][a:b].astype(np.int64)
        z = refs(case, monkeypatch.setenv)[0].means3D[pl, 2].numpy()
        assert (np.diff(z) >= 0).all() and (np.diff(pl)[np.diff(z) == 0] > 0).all()


@pytest.mark.parametrize("case", ["rounds16", "rounds2064"])
def test_several_lds_rounds(case, monkeypatch):
    """A part of a cell with more entries than one LDS round of the finish (3072): 5000 in each part of the only cell (lists of 1250: the
    compositing kernel's slow path), 3400 in one part of a sixteen-tile cell (lists of 850: the 513 - 1024 branch, tied depths)."""
    got, n = check_case(case, monkeypatch.setenv, radix_image=case != "rounds16")
    assert n.max() == {"rounds16": 1250, "rounds2064": 850}[case] and got["I"] == int(n.sum())


def test_capacity_below_the_count_is_clamped_and_redone(monkeypatch):
    """A second forward of the shape speculates with headroom; one whose scene outgrew the speculative capacity (scale modifier 0.15, then
    1.0) runs the two kernels clamped to the capacity and is redone at the exact size."""
    sc, bucket, radix = refs("tiles33", monkeypatch.setenv)
    second = run(sc, "cells", monkeypatch.setenv, before=(1.0,), exact=False)
    assert second["cap"] > second["I"], "the second forward speculates with headroom"
    assert_same_bits(second, bucket, "second forward vs bucket")
    sc, bucket, radix = refs("big_splats", monkeypatch.setenv)
    redo = run(sc, "cells", monkeypatch.setenv, before=(0.15,), exact=False, profile=True)
    print(redo["ran"])
    assert redo["cap"] == redo["I"], "the redone forward is laid out exactly"
    assert redo["ran"].get("cell_finish_kernel") == 2, "clamped, then redone"
    assert_same_bits(redo, bucket, "overflow redo vs bucket")
    assert_same_bits(redo, radix, "overflow redo vs radix")


def test_same_scene_twice(monkeypatch):
    """The arrival order inside a segment varies from run to run; what a forward and its backward leave behind does not."""
    sc, bucket, radix = refs("lengths1040", monkeypatch.setenv)
    first = run(sc, "cells", monkeypatch.setenv)
    again = run(sc, "cells", monkeypatch.setenv, before=(1.0,), exact=False)
    assert_same_bits(again, first, "second run vs first")
    assert_same_bits(first, bucket, "first run vs bucket")
