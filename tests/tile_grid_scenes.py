"""Scenes and the regime table of the large tile grids (tests/test_tile_grids_host.py, tests/test_gpu_tile_grids.py).

What the forward's binning does depends on the tile grid: the bits of a tile id (common.h tile_bits), the partition passes and their digit
widths (tile_digit_width), the key bits the passes leave free for depth buckets (path_policy.h seg_dbits) — which decide what every forced
DAS3R_BINNING resolves to —, and whether the emission may read the packed rectangles (buffers.h rect32(): at most 255 tiles per axis).
SHAPES holds the smallest image of each regime; the functions below RESTATE the formulas of common.h and path_policy.h in Python (they
are not read from the library: tests/test_tile_grids_host.py holds them against it and against REGIMES, the table worked out by hand),
and the GPU tests take their expected plan from here, never from what a run happened to do.

Every scene is a few thousand splats on a mostly empty image: make_scene's random splats plus splats placed (placed_scene) on the tiles
where a wrong digit width, a truncated tile coordinate or a wrong block -> tile map would show."""
import numpy as np
import torch

TILE = 16
SWITCHES = ("radix", "local", "seg", "seg3", "bucket", "cells")                       # DAS3R_BINNING
FORCED = {"radix": -1, "local": 1, "seg": 2, "seg3": 3, "bucket": 4, "cells": 5}       # kernel_choice.h Switches::binning
BUCKET_LOCAL_DBITS = 2                                                                 # path_policy.h
LOCAL_MAX = 1024                                                                       # common.h: longest list the forward kernels order in LDS

# name -> (W, H): the smallest image that reaches the regime
SHAPES = {
    "edge255": (4080, 32),     # 255 x 2: the last shape on the packed path; bx1 == 255 must survive its 8 bits
    "wide256": (4085, 35),     # 256 x 3, ragged: the first shape on the records path (x)
    "tall258": (35, 4117),     # 3 x 258: the same in y
    "sq14": (2048, 2048),      # 128 x 128 = 2^14 tiles: the highest tile id is 2^14 - 1
    "uhd": (3840, 2160),       # 240 x 135
    "full16": (4096, 4080),    # 256 x 255: a tile id fills the sixteen bits of two passes
    "three17": (4112, 4096),   # 257 x 256: three partition passes
}

# Worked out by hand from common.h and path_policy.h (free = 8 * passes - tbits key bits beside the tile id):
#   bucket holds with free >= 2, else the local order; cells where bucket holds and passes <= 2, else where bucket falls;
#   seg needs free >= 1 in the tile passes, seg3 one more pass (at most three in all) — neither falls to the local order: the global sort.
# plan = (kind, onesweep_pass_kernel launches of one forward): the global sort takes four depth passes + the tile passes, cells none.
REGIMES = {
    "edge255": dict(tiles=(255, 2), tbits=9, passes=2, digits=(5, 4), free=7,
                    plans=dict(radix=("radix", 6), local=("local", 2), seg=("seg", 2), seg3=("seg", 3), bucket=("bucket", 2), cells=("cells", 0))),
    "wide256": dict(tiles=(256, 3), tbits=10, passes=2, digits=(5, 5), free=6,
                    plans=dict(radix=("radix", 6), local=("local", 2), seg=("seg", 2), seg3=("seg", 3), bucket=("bucket", 2), cells=("cells", 0))),
    "tall258": dict(tiles=(3, 258), tbits=10, passes=2, digits=(5, 5), free=6,
                    plans=dict(radix=("radix", 6), local=("local", 2), seg=("seg", 2), seg3=("seg", 3), bucket=("bucket", 2), cells=("cells", 0))),
    "sq14": dict(tiles=(128, 128), tbits=14, passes=2, digits=(7, 7), free=2,
                 plans=dict(radix=("radix", 6), local=("local", 2), seg=("seg", 2), seg3=("seg", 3), bucket=("bucket", 2), cells=("cells", 0))),
    "uhd": dict(tiles=(240, 135), tbits=15, passes=2, digits=(8, 7), free=1,
                plans=dict(radix=("radix", 6), local=("local", 2), seg=("seg", 2), seg3=("seg", 3), bucket=("local", 2), cells=("local", 2))),
    "full16": dict(tiles=(256, 255), tbits=16, passes=2, digits=(8, 8), free=0,
                   plans=dict(radix=("radix", 6), local=("local", 2), seg=("radix", 6), seg3=("seg", 3), bucket=("local", 2), cells=("local", 2))),
    "three17": dict(tiles=(257, 256), tbits=17, passes=3, digits=(6, 6, 5), free=7,
                    plans=dict(radix=("radix", 7), local=("local", 3), seg=("seg", 3), seg3=("radix", 7), bucket=("bucket", 3), cells=("bucket", 3))),
}


# ------------------------------------------------------------------------------------------------ common.h and path_policy.h, restated
def grid(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def tile_bits(ntiles):
    b = 0
    while (1 << b) < ntiles:
        b += 1
    return max(b, 1)


def tile_passes(tbits):
    return (tbits + 7) // 8


def digit_widths(tbits):
    """The tile bits split evenly over the passes (tile_digit_width), the last digit taking what is left."""
    passes = tile_passes(tbits)
    dw = (tbits + passes - 1) // passes
    out, sh = [], 0
    while sh < tbits:
        out.append(min(dw, tbits - sh))
        sh += dw
    return tuple(out)


def seg_dbits(tbits, passes):
    return 8 * min(passes, 3) - tbits


def forced_plan(tbits, switch):
    """What plan_forward makes of DAS3R_BINNING=switch on a shape's first forward -> (kind, onesweep_pass_kernel launches)."""
    forced, tp = FORCED[switch], tile_passes(tbits)
    bucket_local = seg_dbits(tbits, tp) >= BUCKET_LOCAL_DBITS and forced in (4, 5)
    cells = bucket_local and tp <= 2 and forced == 5
    local = not bucket_local and forced in (1, 4, 5)
    seg_passes = tp + (1 if not bucket_local and forced == 3 else 0)
    seg_bits = seg_dbits(tbits, seg_passes) if seg_passes <= 3 else 0
    seg = bucket_local or (not local and seg_bits > 0 and forced in (2, 3))
    if cells:
        return "cells", 0
    if bucket_local:
        return "bucket", tp
    if local:
        return "local", tp
    if seg:
        return "seg", seg_passes
    return "radix", 4 + tp


def regime(name):
    """REGIMES' entry of a shape, from the formulas."""
    W, H = SHAPES[name]
    tx, ty = grid(W, H)
    tbits = tile_bits(tx * ty)
    return dict(tiles=(tx, ty), tbits=tbits, passes=tile_passes(tbits), digits=digit_widths(tbits), free=seg_dbits(tbits, tile_passes(tbits)),
                plans={s: forced_plan(tbits, s) for s in SWITCHES})


def packed_rectangles(name):
    """buffers.h rect32(): the emission reads the packed 8-bit rectangles only while neither axis has more than 255 tiles."""
    tx, ty = grid(*SHAPES[name])
    return tx <= 255 and ty <= 255


# ------------------------------------------------------------------------------------------------------------------------------ scenes
def placed_scene(W, H, counts, seed, zlevels=None, pixels=None, s_px=(0.4, 0.6), opacity=0.05):
    """Small splats (footprints of at most 9 pixels across) on the centres of chosen tiles: counts = {tile id: entries of its list}.
    pixels = {(x, y): splats}: further splats centred on those pixels (with a larger s_px: footprints that cross a tile border or the image edge)."""
    from das3r_amd.synth import Scene, make_scene
    tiles_x = (W + 15) // 16
    tile = torch.tensor([t for t, n in counts.items() for _ in range(n)], dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    tile = tile[torch.randperm(tile.numel(), generator=g)]   # (ids and tiles unrelated)
    px = (tile % tiles_x).to(torch.float32) * 16.0 + 7.5
    py = (tile // tiles_x).to(torch.float32) * 16.0 + 7.5
    if pixels:
        at = torch.tensor([xy for xy, n in pixels.items() for _ in range(n)], dtype=torch.float32).reshape(-1, 2)
        at = at[torch.randperm(at.shape[0], generator=g)]
        px, py = torch.cat([px, at[:, 0]]), torch.cat([py, at[:, 1]])
    # (a field of view no wider than the 128-pixel image's, along the longer axis: footprints at the border stay inside their tile)
    focal = max(100.0, max(W, H) / 1.28)
    sc = make_scene(P=int(px.numel()), W=W, H=H, focal=focal, sh_degree=1, seed=seed, s_px=s_px, opacity=opacity)
    z = sc.means3D[:, 2].clone()
    if zlevels:   # a few depth values: equal depths with different ids in every segment
        z = 2.0 + 6.0 * torch.randint(0, zlevels, z.shape, generator=g).to(torch.float32) / zlevels
    means = torch.stack([(px - (W - 1) / 2.0) / focal * z, (py - (H - 1) / 2.0) / focal * z, z], 1).contiguous()
    scales = (sc.scales * (z / sc.means3D[:, 2])[:, None]).contiguous()
    return Scene(**{**sc.__dict__, "means3D": means, "scales": scales})


def concat_scenes(first, *more):
    """One scene of several over the same camera: the per-splat tensors one after the other, everything else the first's."""
    from das3r_amd.synth import Scene
    per_splat = ("means3D", "scales", "rotations", "opacities", "shs")
    for sc in more:
        assert (sc.W, sc.H, sc.tanfovx, sc.tanfovy, sc.sh_degree) == (first.W, first.H, first.tanfovx, first.tanfovy, first.sh_degree)
    return Scene(**{**first.__dict__, **{k: torch.cat([getattr(s, k) for s in (first, *more)], 0).contiguous() for k in per_splat}})


def named_tiles(name):
    """The tiles a shape's scene must reach, {tile id: why}: the first and the last, both sides of column and row 254 | 255 | 256 where the grid has
    them, and both sides of every digit boundary of the tile id — of the shape's own digits, of the eight-bit digits a wrong width would
    take, and of the id's top bit."""
    tx, ty = grid(*SHAPES[name])
    n = tx * ty
    tbits = tile_bits(n)
    out = {0: "first", n - 1: "last"}
    for c in (253, 254, 255, 256, 257):
        if c < tx:
            out.setdefault(min(1, ty - 1) * tx + c, f"column {c}")
        if c < ty:
            out.setdefault(c * tx + min(1, tx - 1), f"row {c}")
    shifts, sh = set(), 0
    for w in digit_widths(tbits)[:-1]:
        sh += w
        shifts.add(sh)
    for sh in sorted(shifts | {8, 16, tbits - 1}):
        if 0 < sh and (1 << sh) < n:
            out.setdefault((1 << sh) - 1, f"below 2^{sh}")
            out.setdefault(1 << sh, f"2^{sh}")
    return out


def long_tiles(name):
    """(tile of the 300-entry list, tile of the 1100-entry list): high tile ids that are no named tile (the last tile's list stays short)"""
    tx, ty = grid(*SHAPES[name])
    taken, free = named_tiles(name), []
    t = tx * ty - 3
    while len(free) < 2:
        if t not in taken:
            free.append(t)
        t -= 2
    return free[0], free[1]


LIST_MID, LIST_LONG = 300, 1100   # one list in 257 - 512 (local_order_tile's rank branch), one beyond LOCAL_MAX (its slow path, in global memory)
ZLEVELS = 5
SEEDS = {name: 900 + i for i, name in enumerate(SHAPES)}
_SCENES = {}


def crossing_pixels(name):
    """{(x, y): splats} of the larger placed splats: across column 255 | 256 (x = 4096) and row 255 | 256 where the grid has them, and over the
    right and the bottom image edge (their 3-sigma square is clipped there: rmaxx == tiles_x, rmaxy == tiles_y)."""
    W, H = SHAPES[name]
    tx, ty = grid(W, H)
    out = {}
    if tx > 256:
        out[(4095.5, min(H - 1, 24) + 0.0)] = 3
        out[(4094.0, H / 2.0)] = 2
    if ty > 256:
        out[(min(W - 1, 24) + 0.0, 4095.5)] = 3
        out[(W / 2.0, 4094.0)] = 2
    out[(W - 2.0, H / 3.0)] = 2            # over the right edge
    out[(W / 3.0, H - 2.0)] = 2            # over the bottom edge
    out[(W - 3.0, H - 3.0)] = 2            # over both, in the last tile
    return out


def scene(name, long_list=True):
    """The shape's scene, built once and never written to: 2500 random splats of 1 - 20 pixels, 3 - 6 small splats with tied depths on
    every named tile, the two long lists, and the crossing splats.  long_list=False: without the list beyond LOCAL_MAX (a shape whose lists
    all fit in LDS keeps the local order on its second forward)."""
    from das3r_amd.synth import make_scene
    key = (name, long_list)
    if key not in _SCENES:
        W, H = SHAPES[name]
        seed = SEEDS[name]
        counts = {t: 3 + t % 4 for t in named_tiles(name)}
        mid, long_ = long_tiles(name)
        counts[mid] = LIST_MID
        if long_list:
            counts[long_] = LIST_LONG
        focal = max(W, H) / 1.28
        random = make_scene(P=2500, W=W, H=H, focal=focal, sh_degree=1, seed=seed, s_px=(1.0, 20.0))
        placed = placed_scene(W, H, counts, seed + 100, zlevels=ZLEVELS)
        crossing = placed_scene(W, H, {}, seed + 200, zlevels=ZLEVELS, pixels=crossing_pixels(name), s_px=(3.0, 5.0), opacity=0.3)
        assert placed.tanfovx == random.tanfovx and crossing.tanfovy == random.tanfovy
        _SCENES[key] = concat_scenes(random, placed, crossing)
    return _SCENES[key]


def stacked_scene(name, tiles, per_tile=4):
    """`per_tile` splats of a dozen pixels at increasing depths on the centre of each tile, opacity 0.3: T falls through 1/2 inside every
    stack.  (The float64 dense references hold [pixels, splats] matrices: a handful of splats is what a 16.8 M-pixel image leaves room for.)"""
    from das3r_amd.synth import Scene
    W, H = SHAPES[name]
    sc = placed_scene(W, H, {t: per_tile for t in tiles}, SEEDS[name] + 300, s_px=(2.0, 3.0), opacity=0.3)
    z = sc.means3D[:, 2]
    znew = 2.0 + torch.arange(sc.P, dtype=torch.float32) * 0.25    # all depths differ
    f = znew / z
    means = sc.means3D * f[:, None]
    means[:, 2] = znew
    return Scene(**{**sc.__dict__, "means3D": means.contiguous(), "scales": (sc.scales * f[:, None]).contiguous()})


MODE = dict(colors_precomp=False, cov3D_precomp=False, scale_modifier=1.0)
_ORACLE = {}


def oracle(name):
    """The C oracle's forward + backward of scene(name) — (color, radii, grads, saved state) —, computed once per shape and shared."""
    from tests import util
    if name not in _ORACLE:
        _ORACLE[name] = util.run_oracle(scene(name), MODE)
    return _ORACLE[name]


def upstream_rects(name, xy, radii):
    """upstream:auxiliary.h getRect of every splat, from the oracle's pixel centres and radii -> (rminx, rminy, rmaxx, rmaxy) int64 arrays"""
    tx, ty = grid(*SHAPES[name])
    x, y, r = xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32), radii.astype(np.float32)
    lo = lambda c, lim: np.clip(((c - r) / np.float32(TILE)).astype(np.int64), 0, lim)
    hi = lambda c, lim: np.clip(((c + r + np.float32(TILE - 1)) / np.float32(TILE)).astype(np.int64), 0, lim)
    return lo(x, tx), lo(y, ty), hi(x, tx), hi(y, ty)
