"""CPU tests of tests/tile_grid_scenes.py: (1) its regime table — bits of a tile id, partition passes, digit widths, free key bits and what
every forced DAS3R_BINNING resolves to, per shape — restated from common.h and path_policy.h, held against the table worked out by hand
and against the library's host entry points (das3r_debug_path_policy_plan, das3r_debug_seg_dbits, das3r_raster_get_layout); (2) its
scenes, from the C oracle's saved state: they reach the tiles, rectangles, list lengths and ties they are there for.  The GPU tests
(tests/test_gpu_tile_grids.py) take their expected plans from the table asserted here."""
import ctypes as C

import numpy as np
import pytest

from tests import tile_grid_scenes as tg

NAMES = list(tg.SHAPES)


def _align(n, a=256):
    return (n + a - 1) // a * a


# --------------------------------------------------------------------------------------------------------------------- 1. the regime table
@pytest.mark.parametrize("name", NAMES)
def test_formulas_give_the_hand_table(name):
    assert tg.regime(name) == tg.REGIMES[name]


def test_the_shapes_are_the_regimes_they_are_named_for():
    R = tg.REGIMES
    assert tg.packed_rectangles("edge255") and R["edge255"]["tiles"][0] == 255, "the last grid on the packed path"
    assert not tg.packed_rectangles("wide256") and R["wide256"]["tiles"] == (256, 3) and tg.SHAPES["wide256"][0] % 16 and tg.SHAPES["wide256"][1] % 16
    assert not tg.packed_rectangles("tall258") and R["tall258"]["tiles"][1] > 255 >= R["tall258"]["tiles"][0]
    assert R["sq14"]["tiles"][0] * R["sq14"]["tiles"][1] == 1 << 14 and tg.packed_rectangles("sq14")
    assert [R[n]["free"] for n in ("sq14", "uhd", "full16")] == [2, 1, 0], "bucket / cells at their limit, one bucket bit for seg, none"
    assert not tg.packed_rectangles("full16") and not tg.packed_rectangles("three17") and tg.packed_rectangles("uhd")
    assert R["three17"]["passes"] == 3 and all(R[n]["passes"] == 2 for n in NAMES if n != "three17")
    assert sorted({R[n]["tbits"] for n in NAMES}) == [9, 10, 14, 15, 16, 17]
    # a partition that took eight bits a pass instead of tile_digit_width would agree with the emission's histograms on two shapes only
    eight = lambda tbits: (8,) * (tbits // 8) + ((tbits % 8,) if tbits % 8 else ())
    assert [n for n in NAMES if R[n]["digits"] == eight(R[n]["tbits"])] == ["uhd", "full16"]
    for n in NAMES:
        assert sum(R[n]["digits"]) == R[n]["tbits"] and max(R[n]["digits"]) <= 8 and len(R[n]["digits"]) == R[n]["passes"]
        assert max(tg.SHAPES[n]) * min(tg.SHAPES[n]) <= 4112 * 4096, "the largest image is 16.8 M pixels"


@pytest.mark.parametrize("name", NAMES)
def test_library_layout_has_the_tiles_and_the_passes(name, hip_lib):
    """das3r_raster_get_layout: the image buffer ends in 8 + 4 bytes per tile (ranges, tile order), and the list buffer the layout calls
    point_list is the fourth of the binning buffer's 4-byte arrays when the tile passes are odd in number, the third when even (api.hip)."""
    from das3r_amd import _lib
    W, H = tg.SHAPES[name]
    tx, ty = tg.REGIMES[name]["tiles"]
    P, cap = 1000, 12345
    L = _lib.layout(P, cap, W, H)
    assert L["ranges"] == 2 * _align(4 * W * H)
    assert L["img_bytes"] - L["ranges"] == _align(8 * tx * ty) + _align(4 * tx * ty)
    assert L["point_list"] == (3 if tg.REGIMES[name]["passes"] & 1 else 2) * _align(4 * cap)


def _library_plan(lib, name, switch):
    """plan_forward of a shape's first forward with DAS3R_BINNING=switch forced, on a fresh state -> (kind, onesweep launches), raw plan"""
    from das3r_amd import _lib
    W, H = tg.SHAPES[name]
    tx, ty = tg.grid(W, H)
    tbits = tg.tile_bits(tx * ty)
    tp = tg.tile_passes(tbits)
    s, p = _lib.PathPolicyState(), _lib.PathPolicyPlan()
    lib.das3r_debug_path_policy_fresh(C.byref(s), 0)
    i = _lib.PathPolicyInputs(4000, W, H, tx * ty, tbits, tp, 0, 0, tg.FORCED[switch], 1, -1, 0)
    lib.das3r_debug_path_policy_plan(C.byref(s), C.byref(i), C.byref(p))
    if p.cells:
        kind = ("cells", 0)
    elif p.seg == 2:
        kind = ("bucket", tp)
    elif p.local:
        kind = ("local", tp)
    elif p.seg:
        kind = ("seg", p.seg_passes)
    else:
        kind = ("radix", 4 + tp)
    return kind, p


@pytest.mark.parametrize("switch", tg.SWITCHES)
@pytest.mark.parametrize("name", NAMES)
def test_library_policy_resolves_every_switch_as_the_table_says(name, switch, hip_lib):
    R = tg.REGIMES[name]
    kind, p = _library_plan(hip_lib, name, switch)
    assert kind == R["plans"][switch], (name, switch)
    assert not (p.local and p.seg) and p.speculate == 0 and p.cap == 0, "a first forward never speculates"
    if kind[0] in ("seg", "bucket", "cells"):
        passes = kind[1] if kind[0] == "seg" else R["passes"]
        assert p.seg_passes == passes and p.seg_bits == 8 * passes - R["tbits"] > 0, "the key is as wide as its passes"
    assert hip_lib.das3r_debug_seg_dbits(R["tbits"], R["passes"]) == R["free"]
    assert hip_lib.das3r_debug_seg_dbits(R["tbits"], R["passes"] + 1) == 8 * min(R["passes"] + 1, 3) - R["tbits"]


def test_unforced_first_forward_takes_the_local_order(hip_lib):
    """No switch: a shape's first forward plans the local order at every grid (tests/test_gpu_tile_grids.py part b)."""
    from das3r_amd import _lib
    for name in NAMES:
        W, H = tg.SHAPES[name]
        R = tg.REGIMES[name]
        s, p = _lib.PathPolicyState(), _lib.PathPolicyPlan()
        hip_lib.das3r_debug_path_policy_fresh(C.byref(s), 0)
        i = _lib.PathPolicyInputs(4000, W, H, R["tiles"][0] * R["tiles"][1], R["tbits"], R["passes"], 0, 0, 0, 1, -1, 0)
        hip_lib.das3r_debug_path_policy_plan(C.byref(s), C.byref(i), C.byref(p))
        assert (p.local, p.seg, p.cells) == (1, 0, 0), name


# ---------------------------------------------------------------------------------------------------------------------------- 2. the scenes
def _lengths(S):
    return (S["ranges"][:, 1].astype(np.int64) - S["ranges"][:, 0].astype(np.int64))


@pytest.mark.parametrize("name", NAMES)
def test_scene_reaches_what_it_is_there_for(name):
    sc = tg.scene(name)
    _, radii, _, S = tg.oracle(name)
    tx, ty = tg.REGIMES[name]["tiles"]
    ntiles = tx * ty
    n = _lengths(S)
    assert len(n) == ntiles and 3500 <= sc.P <= 6000
    assert S["num_rendered"] == int(n.sum()) <= 384 * ntiles, "mean list below LOCAL_AVG: the unforced plan is the local order"
    assert (n == 0).any() or ntiles < 1000, "empty tiles keep their zeroed ranges"
    # the named tiles
    for t, why in tg.named_tiles(name).items():
        assert n[t] >= 3, f"{name}: tile {t} ({why}) has {n[t]} entries"
    # the two long lists, at high tile ids; every other list fits in LDS
    mid, long_ = tg.long_tiles(name)
    assert 257 <= n[mid] <= 512 and n[long_] > tg.LOCAL_MAX and min(mid, long_) > ntiles - 16, (n[mid], n[long_])
    assert np.delete(n, long_).max() <= tg.LOCAL_MAX and n[ntiles - 1] < 64
    # rectangles, rebuilt from the oracle's pixel centres and radii
    vis = radii > 0
    x0, y0, x1, y1 = (a[vis] for a in tg.upstream_rects(name, S["xy"], radii))
    assert np.array_equal(((x1 - x0) * (y1 - y0)).astype(np.uint32), S["tiles_touched"][vis].astype(np.uint32)), "the rectangles are the oracle's"
    assert (x1 == tx).any() and (y1 == ty).any() and ((x1 == tx) & (y1 == ty)).any(), "squares clipped by the right and the bottom edge"
    if tx > 255:
        assert ((x1 == tx) & (x1 > 255)).any(), "rmaxx == tiles_x does not fit eight bits"
    if ty > 255:
        assert ((y1 == ty) & (y1 > 255)).any()
    if tx > 256:
        assert ((x0 <= 255) & (x1 >= 257) & (x1 - x0 <= 6)).sum() >= 3, "small squares across column 255 | 256"
    if ty > 256:
        assert ((y0 <= 255) & (y1 >= 257) & (y1 - y0 <= 6)).sum() >= 3
    # the packed word (preprocess.hip: x0 | x1 << 8 | y0 << 16 | y1 << 24) holds these rectangles where rect32() (buffers.h) lets the emission read it, and
    # nowhere else: an emission that read it on the larger grids would bin other rectangles than these
    word = (x0 | (x1 << 8) | (y0 << 16) | (y1 << 24)) & 0xFFFFFFFF
    unpacked = (word & 255, (word >> 16) & 255, (word >> 8) & 255, word >> 24)
    assert all(np.array_equal(a, b) for a, b in zip(unpacked, (x0, y0, x1, y1))) == tg.packed_rectangles(name)
    if name == "edge255":
        assert x1.max() == 255 and ((x1 == 255) & (x0 < 255)).any(), "bx1 == 255 in the packed word"
    # ties: equal depths with different ids inside one list, in id order
    z = sc.means3D[:, 2].numpy()
    for t in (mid, long_, ntiles - 1):
        a, b = S["ranges"][t]
        pl = S["point_list"][a:b].astype(np.int64)
        dz, did = np.diff(z[pl]), np.diff(pl)
        assert (dz >= 0).all() and (did[dz == 0] > 0).all(), f"{name}: tile {t}"
        assert (dz == 0).sum() >= 100 or t == ntiles - 1, f"{name}: tile {t}: {tg.ZLEVELS} depth values over hundreds of entries"


def test_scene_without_the_long_list_differs_by_that_list_only():
    a, b = tg.scene("uhd"), tg.scene("uhd", long_list=False)
    assert a.P - b.P == tg.LIST_LONG and a.W == b.W and a.H == b.H
